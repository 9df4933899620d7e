"""The fp64 restatement of tests/vision_tower_cases.py against the goldens of the unmodified reference image encoder
(tests/golden/vision_tower_*.npz, tools/make_vision_tower_golden.py), the parameter layout of vision_tower.ImageEncoderViT against the key
list the goldens record, the sensitivity of the fixtures to every term a kernel could drop, the host-only entry points of the fused
relative-position attention (its route query over the whole family, and the coverage of the GPU test's grid list per route class), the
kernel's key-coordinate arithmetic and the window split.  No GPU.

Bar: 2e-5 max(1, max|ref|), the one tests/test_bev_backbone_restatements.py holds fp64 restatements to against fp32-torch goldens."""
import ctypes
import os
from functools import partial

import numpy as np
import pytest
import torch

import vision_tower_cases as VC
from lidar_vision_vqa_amd import _ffi
from lidar_vision_vqa_amd import vision_tower as VT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 2e-5
GPU_BAR = 1e-3
SMALL = [n for n in VC.CASES if n != "vit_b_1024"]


def golden(name):
    return np.load(os.path.join(GOLDEN, VC.golden_name(name)))


def build(name):
    cfg = VC.CASES[name][0]
    if name == "vit_b_1024":
        return VT.build_sam_vit_b()
    return VT.ImageEncoderViT(**cfg, qkv_bias=True, use_rel_pos=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))


@pytest.mark.parametrize("name", list(VC.CASES))
def test_restatement_agrees_with_the_reference_module(name):
    want = golden(name)["out"]
    ref = VC.case_ref(name)
    assert ref.shape == want.shape and want.dtype == np.float32
    mag = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(ref - want).max())
    print(f"{name}: restatement vs golden {err:.3e} (bar {BAR * mag:.3e}, max|ref| {mag:.3f})")
    assert err <= BAR * mag
    assert mag > 1.0


def test_restatement_forms_its_bias_from_shifted_tables():
    """bias_terms reads reversed windows of T = q [Rh; Rw]^T (shapes [.., gh] and [.., gw] per query); it agrees with the dense gather
    Rh[y - ky + gh - 1] . q written out here on a non-square grid, where a swap of the two axes would show."""
    gh, gw, dh = 3, 5, 8
    rng = np.random.default_rng(5)
    q = torch.from_numpy(rng.standard_normal((2, 1, gh * gw, dh)))
    rh, rw = torch.from_numpy(rng.standard_normal((2 * gh - 1, dh))), torch.from_numpy(rng.standard_normal((2 * gw - 1, dh)))
    bh, bw = VC.bias_terms(q, rh, rw, gh, gw)
    assert tuple(bh.shape) == (2, 1, gh, gw, gh) and tuple(bw.shape) == (2, 1, gh, gw, gw)
    ys, xs = np.arange(gh), np.arange(gw)
    dense_h = torch.einsum("bnyxc,ykc->bnyxk", q.view(2, 1, gh, gw, dh), rh[ys[:, None] - ys[None, :] + gh - 1])
    dense_w = torch.einsum("bnyxc,xkc->bnyxk", q.view(2, 1, gh, gw, dh), rw[xs[:, None] - xs[None, :] + gw - 1])
    assert float((bh - dense_h).abs().max()) < 1e-12 and float((bw - dense_w).abs().max()) < 1e-12
    d = VC.dense_bias(q.numpy(), rh.numpy(), rw.numpy(), gh, gw)
    assert d.shape == (2, 1, gh * gw, gh * gw)
    assert abs(d[1, 0, 1 * gw + 2, 2 * gw + 4] - float(q[1, 0, gw + 2] @ (rh[1 - 2 + gh - 1] + rw[2 - 4 + gw - 1]))) < 1e-12


@pytest.mark.parametrize("name", list(VC.CASES))
def test_state_dict_keys_order_and_shapes_are_the_reference_s(name):
    g = golden(name)
    want = [(str(k), tuple(int(d) for d in str(s).split(",") if d)) for k, s in zip(g["keys"], g["shapes"])]
    m = build(name)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == want                                                          # same keys, same order, same shapes
    assert got == [(k, tuple(s)) for k, s in VC.state_shapes(VC.CASES[name][0])]
    if name != "vit_b_1024":                                                    # (seeding 95.6 M parameters again would only cost time)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in VC.case_state(name).items()}, strict=True)


def test_default_init_consumes_the_rng_in_torch_s_order():
    """The containers are built in the reference's order: patch_embed.proj, then per block attn.qkv, attn.proj, mlp.lin1, mlp.lin2, then
    the neck convs, net_2, net_3; pos_embed and the rel-pos tables start at zero and take nothing from the generator."""
    import torch.nn as nn
    torch.manual_seed(11)
    ours = build("pad")
    torch.manual_seed(11)
    pe = nn.Conv2d(3, 128, kernel_size=(16, 16), stride=(16, 16), padding=(0, 0))
    qkv, proj, lin1, lin2 = nn.Linear(128, 384), nn.Linear(128, 128), nn.Linear(128, 512), nn.Linear(512, 128)
    assert torch.equal(ours.patch_embed.proj.weight, pe.weight) and torch.equal(ours.patch_embed.proj.bias, pe.bias)
    b0 = ours.blocks[0]
    assert torch.equal(b0.attn.qkv.weight, qkv.weight) and torch.equal(b0.attn.proj.weight, proj.weight)
    assert torch.equal(b0.mlp.lin1.weight, lin1.weight) and torch.equal(b0.mlp.lin2.bias, lin2.bias)
    assert float(ours.pos_embed.detach().abs().max()) == 0.0 and float(b0.attn.rel_pos_h.detach().abs().max()) == 0.0
    assert tuple(b0.attn.rel_pos_h.shape) == (7, 64) and tuple(ours.blocks[1].attn.rel_pos_w.shape) == (19, 64)
    assert b0.window_size == 4 and ours.blocks[1].window_size == 0 and b0.norm1.eps == 1e-6


def test_module_refuses_what_has_no_kernel():
    with pytest.raises(_ffi.LvqError):                                          # CPU tensors: no fallback
        with torch.no_grad():
            build("pad").eval()(torch.zeros(1, 3, 160, 160))
    with pytest.raises(_ffi.LvqError):                                          # train() mode
        build("pad")(torch.zeros(1, 3, 160, 160))


@pytest.mark.parametrize("variant", ["no_rel", "swap", "mask_pad", "no_pos"])
@pytest.mark.parametrize("name", SMALL)
def test_fixtures_notice_every_term(name, variant):
    """A restatement without the term differs from the golden by at least 100 x the GPU bar, so no kernel that ignores it can pass.
    (`resized` has an 8 x 8 grid and windows of 4: nothing is padded there, so masking pad keys changes nothing and is not asked.)"""
    if variant == "mask_pad" and name == "resized":
        assert np.array_equal(VC.case_ref(name, variant), VC.case_ref(name))
        return
    want = golden(name)["out"]
    mag = max(1.0, float(np.abs(want).max()))
    diff = float(np.abs(VC.case_ref(name, variant) - want).max())
    print(f"{name} / {variant}: moves the output by {diff:.3f} (needs {100 * GPU_BAR * mag:.3f})")
    assert diff >= 100 * GPU_BAR * mag


def test_host_only_entry_points():
    L = _ffi.lib()
    ok = L.lvq_attention_relpos_ok
    for shape in ((14, 14, 64), (64, 64, 64), (1, 1, 64), (5, 7, 64)):
        assert ok(*map(ctypes.c_int, shape)) == 1, shape
    for shape in ((14, 14, 80), (65, 14, 64), (14, 65, 64), (0, 4, 64)):
        assert ok(*map(ctypes.c_int, shape)) == 0, shape
    for prec in (1, 3):
        n = L.lvq_attention_relpos_workspace_bytes(*map(ctypes.c_int, (1, 12, 64, 64, 64, prec)))
        assert 0 <= n < 12 * 64 * 64 * 64 * 64 * 4


# ------------------------------------------------------------------------------------------------------------------------------------
# routes of k_attn_relpos<NSPLIT, STAGES>: the query lvq_attention_relpos_plan over the whole family
# ------------------------------------------------------------------------------------------------------------------------------------
LDS_CU = 160 * 1024
LDS_MAX = 122624                # hi + lo, two stages, table stride 191: the grid (64, 63)


def route_class(gh, gw, precision):
    """(precision, K | V stages, one-row): one-row grids (gw % 16 == 0) keep every wave's 16 queries in one grid row (the narrow Rw window);
    on all others a wave spans rows and takes the whole Rw table."""
    return precision, _ffi.attention_relpos_plan(gh, gw, precision)[0], gw % 16 == 0


def test_route_query_over_the_whole_family():
    worst, at = 0, []
    for prec in (1, 3):
        for gh in range(1, 65):
            for gw in range(1, 65):
                stages, nbytes = _ffi.attention_relpos_plan(gh, gw, prec)
                assert stages in (1, 2) and 0 < nbytes <= LDS_CU, (gh, gw, prec, stages, nbytes)
                if nbytes >= worst:
                    at = at + [(gh, gw, prec, stages)] if nbytes == worst else [(gh, gw, prec, stages)]
                    worst = nbytes
    assert worst == LDS_MAX and at == [(64, 63, 3, 2)], (worst, at)
    L = _ffi.lib()
    st, nb = ctypes.c_int(-7), ctypes.c_size_t(12345)
    for args, rc in (((65, 4, 1), -5), ((4, 0, 3), -5), ((4, 4, 2), -1), ((4, 4, 0), -1)):
        assert L.lvq_attention_relpos_plan(*map(ctypes.c_int, args), ctypes.byref(st), ctypes.byref(nb)) == rc, args
        assert (st.value, nb.value) == (-7, 12345)                              # a refusal writes nothing
    assert L.lvq_attention_relpos_plan(*map(ctypes.c_int, (4, 4, 1)), None, ctypes.byref(nb)) == -1
    assert L.lvq_attention_relpos_plan(*map(ctypes.c_int, (4, 4, 1)), ctypes.byref(st), None) == -1


def test_gpu_grid_list_covers_every_route_class():
    """tests/test_gpu_relpos_attention.py runs ROUTE_GRIDS in both precisions.  Every (precision, stages, one-row) class that any grid of
    the family selects must have a grid in that list, and so must the grid of the largest LDS request: if rel_stages changes, this names
    the route that lost its coverage."""
    import test_gpu_relpos_attention as RA
    family, covered = {}, {}
    for prec in (1, 3):
        for gh in range(1, 65):
            for gw in range(1, 65):
                family.setdefault(route_class(gh, gw, prec), (gh, gw))
        for gh, gw in RA.ROUTE_GRIDS:
            covered.setdefault(route_class(gh, gw, prec), (gh, gw))
    print({c: covered.get(c) for c in sorted(family)})
    lost = {c: g for c, g in family.items() if c not in covered}
    assert not lost, f"(precision, stages, one-row) classes no GPU grid runs, with their first grid: {lost}"
    assert (3, 2, False) in family and (1, 2, False) in family and (1, 2, True) in family
    sizes = {g: _ffi.attention_relpos_plan(*g, 3)[1] for g in RA.ROUTE_GRIDS}
    assert max(sizes.values()) == LDS_MAX, sizes


def test_key_coordinates_are_exact_below_4096():
    """coords() of csrc/vit_attention.hip: y = int((float(j) + 0.5f) * (1.0f / gw)) in fp32 is j // gw for every key of every grid width."""
    bad = 0
    for gw in range(1, 65):
        j = np.arange(64 * gw, dtype=np.int64)
        rgw = np.float32(1.0) / np.float32(gw)
        y = ((j.astype(np.float32) + np.float32(0.5)) * rgw)
        assert y.dtype == np.float32
        bad += int((y.astype(np.int64) != j // gw).sum())
    assert bad == 0, bad


# ------------------------------------------------------------------------------------------------------------------------------------
# window_partition / window_unpartition against index loops
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,h,w,c,ws", [(2, 5, 7, 3, 4), (1, 7, 5, 2, 3), (2, 9, 4, 1, 4), (1, 3, 4, 2, 14), (2, 8, 12, 2, 4)])
def test_window_partition_against_index_loops(b, h, w, c, ws):
    x = torch.arange(1, b * h * w * c + 1, dtype=torch.float32).view(b, h, w, c)        # no zero: the padding is told apart
    win, (hp, wp) = VT.window_partition(x, ws)
    nh, nw = -(-h // ws), -(-w // ws)
    assert (hp, wp) == (nh * ws, nw * ws) and tuple(win.shape) == (b * nh * nw, ws, ws, c)
    want = torch.zeros(b * nh * nw, ws, ws, c)
    for bi in range(b):
        for y in range(h):
            for xx in range(w):
                want[(bi * nh + y // ws) * nw + xx // ws, y % ws, xx % ws] = x[bi, y, xx]
    assert torch.equal(win, want)
    back = VT.window_unpartition(win, ws, (hp, wp), (h, w))
    assert back.is_contiguous() and torch.equal(back, x)
    marked = win + 1000.0 * torch.arange(win.shape[0], dtype=torch.float32).view(-1, 1, 1, 1)      # un-partition alone, on window-tagged data
    got = VT.window_unpartition(marked, ws, (hp, wp), (h, w))
    for bi in range(b):
        for y in range(h):
            for xx in range(w):
                assert torch.equal(got[bi, y, xx], marked[(bi * nh + y // ws) * nw + xx // ws, y % ws, xx % ws])


@pytest.mark.parametrize("name", VC.PADDED_BLOCK_CASES)
def test_block_cases_pin_that_pad_keys_are_live(name):
    """The Block cases of tests/test_gpu_vision_tower_modules.py whose windows are padded: masking the pad keys in the fp64 restatement moves
    the result by at least 100 x the bound the GPU module is held to, so a kernel chain that masked them could not pass."""
    ref = VC.block_ref(name)
    need = 100 * VC.BLOCK_BOUND * max(1.0, float(np.abs(ref).max()))
    diff = float(np.abs(VC.block_ref(name, "mask_pad") - ref).max())
    print(f"{name}: mask_pad moves the block's output by {diff:.3f} (needs {need:.3f})")
    assert diff >= need
    b, gh, gw, ws = VC.BLOCK_CASES[name][:4]
    assert gh % ws or gw % ws


def test_sub_modules_refuse_cpu_tensors_and_train_mode():
    mods = {"patch": (VT.PatchEmbed(embed_dim=128), (1, 3, 32, 32)), "ln2d": (VT.LayerNorm2d(32), (1, 32, 2, 2)),
            "mlp": (VT.MLPBlock(128, 512), (3, 128)), "attn": (VT.Attention(128, 2, use_rel_pos=True, input_size=(2, 2)), (1, 2, 2, 128)),
            "block": (VT.Block(128, 2, use_rel_pos=True, input_size=(2, 2)), (1, 2, 2, 128))}
    for name, (m, shape) in mods.items():
        with pytest.raises(_ffi.LvqError), torch.no_grad():                    # CPU tensors: no fallback
            m.eval()(torch.zeros(shape))
        with pytest.raises(_ffi.LvqError), torch.no_grad():                    # train() mode
            m.train()(torch.zeros(shape))
        with pytest.raises(_ffi.LvqError):                                     # gradients in reach
            m.eval()(torch.zeros(shape))
