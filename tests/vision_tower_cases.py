"""Host side (torch CPU, fp64) of the vision tower tests: a restatement of the SAM ViT image encoder (deepencoder/sam_vary_sdpa.py:
100-511) written from the module structure, the configurations of the four goldens, their seeded weights and the operands of the
kernel tests.

  state_shapes  [(key, shape)] in the reference's registration order, from the configuration alone
  state         a seeded state_dict: synth.seeded_array per key, with the two kinds of key whose default scale (1 / sqrt(fan_in)) would
                make their term invisible rescaled: `*.rel_pos_h` / `*.rel_pos_w` ~ N(0, 0.25^2), `pos_embed` ~ N(0, 0.5^2)
  encoder       the chain in float64.  Attention forms its bias by the SHIFTED-TABLE identity: T = q [Rh; Rw]^T once per query, and
                query (y, x) reads T_h[y + gh - 1 - ky] and T_w[x + gw - 1 - kx] -- a reversed window of its own row, never a gather of
                Rh[rel_coords] into an [N, N, dh] array.  `variant` switches one term off (the sensitivity tests):
                "no_rel" (tables zeroed), "swap" (h and w tables exchanged), "mask_pad" (pad keys of a window masked), "no_pos"
  attention_ref the kernel's contract on a packed qkv matrix, fp64
  kernel_operands / regime_operands / one_hot_operands   what the kernel tests feed lvq_attention_relpos_bf16
  ln2d, block, logits                                    single steps of the chain, for the module tests
"""
import functools

import numpy as np
import torch
import torch.nn.functional as TF

from lidar_vision_vqa_amd import synth

SMALL = dict(patch_size=16, in_chans=3, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4.0, out_chans=256, global_attn_indexes=(1,))
VIT_B = dict(img_size=1024, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0, out_chans=256, window_size=14,
             global_attn_indexes=(2, 5, 8, 11))
# name -> (config, input shape, weight seed, input seed)
CASES = {
    "pad": (dict(SMALL, img_size=160, window_size=4), (2, 3, 160, 160), 41, 141),
    "w14": (dict(SMALL, img_size=320, window_size=14), (1, 3, 320, 320), 42, 142),
    "resized": (dict(SMALL, img_size=160, window_size=4), (2, 3, 128, 128), 41, 143),
    "vit_b_1024": (VIT_B, (1, 3, 1024, 1024), 44, 144),
}
LN_EPS = 1e-6
REL_STD, POS_STD = 0.25, 0.5


def golden_name(name):
    return f"vision_tower_{name}.npz"


def case_input(name):
    return synth.randn(CASES[name][1], CASES[name][3])


def state_shapes(cfg):
    d, p, heads = cfg["embed_dim"], cfg["patch_size"], cfg["num_heads"]
    g, oc, hidden = cfg["img_size"] // p, cfg["out_chans"], int(cfg["embed_dim"] * cfg["mlp_ratio"])
    out = [("pos_embed", (1, g, g, d)), ("patch_embed.proj.weight", (d, cfg["in_chans"], p, p)), ("patch_embed.proj.bias", (d,))]
    for i in range(cfg["depth"]):
        s = g if i in cfg["global_attn_indexes"] else cfg["window_size"]
        b = f"blocks.{i}."
        out += [(b + "norm1.weight", (d,)), (b + "norm1.bias", (d,)), (b + "attn.rel_pos_h", (2 * s - 1, d // heads)),
                (b + "attn.rel_pos_w", (2 * s - 1, d // heads)), (b + "attn.qkv.weight", (3 * d, d)), (b + "attn.qkv.bias", (3 * d,)),
                (b + "attn.proj.weight", (d, d)), (b + "attn.proj.bias", (d,)), (b + "norm2.weight", (d,)), (b + "norm2.bias", (d,)),
                (b + "mlp.lin1.weight", (hidden, d)), (b + "mlp.lin1.bias", (hidden,)), (b + "mlp.lin2.weight", (d, hidden)),
                (b + "mlp.lin2.bias", (d,))]
    out += [("neck.0.weight", (oc, d, 1, 1)), ("neck.1.weight", (oc,)), ("neck.1.bias", (oc,)), ("neck.2.weight", (oc, oc, 3, 3)),
            ("neck.3.weight", (oc,)), ("neck.3.bias", (oc,)), ("net_2.weight", (512, 256, 3, 3)), ("net_3.weight", (1024, 512, 3, 3))]
    return out


def seeded(key, shape, seed):
    a = synth.seeded_array(key, tuple(shape), seed)
    std = REL_STD if key.endswith(("rel_pos_h", "rel_pos_w")) else POS_STD if key == "pos_embed" else None
    if std is not None:                                  # seeded_array scaled these by 1 / sqrt(prod(shape[1:]))
        a = (a.astype(np.float64) * (np.sqrt(float(np.prod(shape[1:]))) * std)).astype(np.float32)
    return a


def state(cfg, seed):
    return {k: seeded(k, s, seed) for k, s in state_shapes(cfg)}


@functools.lru_cache(maxsize=None)
def case_state(name):
    return state(CASES[name][0], CASES[name][2])


# --------------------------------------------------------------------------------------------------------------------------------
# fp64 restatement
# --------------------------------------------------------------------------------------------------------------------------------
def _d(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def resized_rel(table, size):
    """A [L, dh] table at length 2 size - 1: linear resize in fp32 (as the reference computes it) when L differs."""
    t = torch.from_numpy(np.asarray(table, np.float32))
    if t.shape[0] != 2 * size - 1:
        t = TF.interpolate(t.t()[None], size=2 * size - 1, mode="linear")[0].t()
    return t.double()


def resized_pos(pos, g):
    t = torch.from_numpy(np.asarray(pos, np.float32))
    if t.shape[1] != g:
        t = TF.interpolate(t.permute(0, 3, 1, 2), size=(g, g), mode="bicubic", antialias=True, align_corners=False).permute(0, 2, 3, 1)
    return t.double()


def bias_terms(q, rel_h, rel_w, gh, gw):
    """q [nb, H, gh * gw, dh], tables [2 g - 1, dh] -> (bh [nb, H, gh, gw, gh], bw [nb, H, gh, gw, gw]) by the shifted-table identity:
    bh[.., y, x, ky] = T_h[.., y, x, y + gh - 1 - ky] with T_h = q Rh^T -- the reversed window [y, y + gh) of the query's own row."""
    nb, nh = q.shape[:2]
    th = (q @ rel_h.t()).view(nb, nh, gh, gw, 2 * gh - 1)
    tw = (q @ rel_w.t()).view(nb, nh, gh, gw, 2 * gw - 1)
    bh = torch.stack([th[:, :, y, :, y:y + gh].flip(-1) for y in range(gh)], dim=2)
    bw = torch.stack([tw[:, :, :, x, x:x + gw].flip(-1) for x in range(gw)], dim=3)
    return bh, bw


def grid_attention(q, k, v, rel_h, rel_w, gh, gw, scale, key_mask=None):
    """softmax(scale q k^T + bias) v per head (a loop: one [N, N] fp64 array at a time), q / k / v [nb, H, N, dh]."""
    nb, nh, n, dh = q.shape
    out = torch.empty_like(q)
    for h in range(nh):
        bh, bw = bias_terms(q[:, h:h + 1], rel_h, rel_w, gh, gw)
        s = (q[:, h] @ k[:, h].transpose(1, 2)) * scale
        s = s + (bh[:, 0, :, :, :, None] + bw[:, 0, :, :, None, :]).reshape(nb, n, n)
        if key_mask is not None:
            s = s.masked_fill(~key_mask[:, None, :], float("-inf"))
        out[:, h] = torch.softmax(s, dim=-1) @ v[:, h]
    return out


def attention_ref(qkv, rel_h, rel_w, batch, n_heads, gh, gw, dh, scale):
    """The kernel's contract: qkv [batch * gh * gw, 3 * n_heads * dh] (column = part * H * dh + h * dh + e) -> [batch * gh * gw, H * dh], fp64."""
    n = gh * gw
    t = _d(qkv).view(batch, n, 3, n_heads, dh).permute(2, 0, 3, 1, 4)
    o = grid_attention(t[0], t[1], t[2], _d(rel_h), _d(rel_w), gh, gw, scale)
    return o.permute(0, 2, 1, 3).reshape(batch * n, n_heads * dh).numpy()


def dense_bias(q, rel_h, rel_w, gh, gw):
    """[nb, H, N, N] fp64 bias of q [nb, H, N, dh] (what the dense-bias route of lvq_attention_bf16 is handed)."""
    bh, bw = bias_terms(_d(q), _d(rel_h), _d(rel_w), gh, gw)
    n = gh * gw
    return (bh[..., :, None] + bw[..., None, :]).reshape(q.shape[0], q.shape[1], n, n).numpy()


def _windows(x, ws):
    b, h, w, c = x.shape
    hp, wp = -(-h // ws) * ws, -(-w // ws) * ws
    x = TF.pad(x, (0, 0, 0, wp - w, 0, hp - h))
    return x.view(b, hp // ws, ws, wp // ws, ws, c).transpose(2, 3).reshape(-1, ws, ws, c), hp, wp


def block(sd, pre, x, heads, ws, variant=None):
    """One Block on x [B, gh, gw, d] fp64 with the state's `pre` keys; ws = 0 is a global block."""
    b, gh, gw, d = x.shape
    dh = d // heads
    h = TF.layer_norm(x, (d,), _d(sd[pre + "norm1.weight"]), _d(sd[pre + "norm1.bias"]), LN_EPS)
    mask = None
    if ws > 0:
        h, hp, wp = _windows(h, ws)
        if variant == "mask_pad":
            mask = _windows(torch.ones(b, gh, gw, 1, dtype=torch.float64), ws)[0].reshape(-1, ws * ws) > 0
    nb, sh, sw = h.shape[:3]
    qkv = (h.reshape(nb, sh * sw, d) @ _d(sd[pre + "attn.qkv.weight"]).t() + _d(sd[pre + "attn.qkv.bias"])).view(nb, sh * sw, 3, heads, dh)
    q, k, v = qkv.permute(2, 0, 3, 1, 4)
    rh, rw = resized_rel(sd[pre + "attn.rel_pos_h"], sh), resized_rel(sd[pre + "attn.rel_pos_w"], sw)
    if variant == "no_rel":
        rh, rw = torch.zeros_like(rh), torch.zeros_like(rw)
    elif variant == "swap":
        rh, rw = rw, rh
    o = grid_attention(q, k, v, rh, rw, sh, sw, dh ** -0.5, mask).permute(0, 2, 1, 3).reshape(nb, sh, sw, d)
    if ws > 0:
        o = o.view(b, hp // ws, wp // ws, ws, ws, d).transpose(2, 3).reshape(b, hp, wp, d)[:, :gh, :gw]
    x = x + o @ _d(sd[pre + "attn.proj.weight"]).t() + _d(sd[pre + "attn.proj.bias"])
    m = TF.layer_norm(x, (d,), _d(sd[pre + "norm2.weight"]), _d(sd[pre + "norm2.bias"]), LN_EPS)
    m = TF.gelu(m @ _d(sd[pre + "mlp.lin1.weight"]).t() + _d(sd[pre + "mlp.lin1.bias"]))
    return x + m @ _d(sd[pre + "mlp.lin2.weight"]).t() + _d(sd[pre + "mlp.lin2.bias"])


def ln2d(x, w, b):
    u = x.mean(1, keepdim=True)
    s = ((x - u) ** 2).mean(1, keepdim=True)
    return (x - u) / torch.sqrt(s + LN_EPS) * _d(w)[:, None, None] + _d(b)[:, None, None]


def encoder(cfg, sd, x, variant=None):
    """x [B, 3, S, S] -> [B, 1024, S / 64, S / 64], float64 numpy."""
    p = cfg["patch_size"]
    x = TF.conv2d(_d(x), _d(sd["patch_embed.proj.weight"]), _d(sd["patch_embed.proj.bias"]), stride=p).permute(0, 2, 3, 1)
    if variant != "no_pos":
        x = x + resized_pos(sd["pos_embed"], x.shape[1])
    for i in range(cfg["depth"]):
        ws = 0 if i in cfg["global_attn_indexes"] else cfg["window_size"]
        x = block(sd, f"blocks.{i}.", x, cfg["num_heads"], ws, variant)
    x = TF.conv2d(x.permute(0, 3, 1, 2), _d(sd["neck.0.weight"]))
    x = ln2d(x, sd["neck.1.weight"], sd["neck.1.bias"])
    x = ln2d(TF.conv2d(x, _d(sd["neck.2.weight"]), padding=1), sd["neck.3.weight"], sd["neck.3.bias"])
    x = TF.conv2d(x, _d(sd["net_2.weight"]), stride=2, padding=1)
    return TF.conv2d(x, _d(sd["net_3.weight"]), stride=2, padding=1).numpy()


@functools.lru_cache(maxsize=None)
def case_ref(name, variant=None):
    """The restatement's output of a golden case (computed once, shared; callers must not write to it)."""
    out = encoder(CASES[name][0], case_state(name), case_input(name), variant)
    out.setflags(write=False)
    return out


# --------------------------------------------------------------------------------------------------------------------------------
# operands of the kernel tests
# --------------------------------------------------------------------------------------------------------------------------------
def kernel_operands(batch, heads, gh, gw, dh, seed):
    """(qkv [batch * gh * gw, 3 * heads * dh] ~ N(0, 1), rel_h, rel_w ~ N(0, 1 / dh), independent draws): each bias term has unit variance
    like the scaled scores."""
    qkv = synth.randn((batch * gh * gw, 3 * heads * dh), seed)
    return qkv, synth.randn((2 * gh - 1, dh), seed + 1, dh ** -0.5), synth.randn((2 * gw - 1, dh), seed + 2, dh ** -0.5)


REGIMES = ("peaked", "peaked_last", "bias_only", "tables_zero")


def logits(qkv, rel_h, rel_w, batch, heads, gh, gw, dh, scale):
    """[batch, heads, N, N] fp64: scale q k^T + bias, the argument of the softmax (small grids only)."""
    n = gh * gw
    t = _d(qkv).view(batch, n, 3, heads, dh).permute(2, 0, 3, 1, 4)
    return (t[0] @ t[1].transpose(-1, -2)) * scale + torch.from_numpy(dense_bias(t[0].numpy(), rel_h, rel_w, gh, gw))


def regime_operands(regime, batch, heads, gh, gw, dh, seed, margin=30.0):
    """kernel_operands moved out of the unit-variance regime:
      peaked       q scaled by 8: scores and both bias terms have standard deviation 8, the running maximum jumps from key tile to key tile
                   and alpha underflows
      peaked_last  peaked, and the LAST key (in the last, partial key tile when N % 64 != 0) holds every row's maximum by at least `margin`:
                   every q has channel 0 = 8, every k channel 0 = 0 except the last key's, which is the smallest multiple of 8 that gives
                   the margin in fp64 on the bf16-rounded operands (so it holds in both operand forms)
      bias_only    k = 0: the output is softmax(bias) v, no score dilutes a table-index error
      tables_zero  rel_h = rel_w = 0: plain attention"""
    qkv, rh, rw = (a.copy() for a in kernel_operands(batch, heads, gh, gw, dh, seed))
    n, d = gh * gw, heads * dh
    if regime in ("peaked", "peaked_last"):
        qkv[:, :d] *= 8.0
    if regime == "peaked_last":
        v = qkv.reshape(batch, n, 3, heads, dh)
        v[:, :, 0, :, 0] = 8.0
        v[:, :, 1, :, 0] = 0.0
        rnd = lambda a: torch.from_numpy(a).to(torch.bfloat16).float().numpy()
        lg = logits(rnd(qkv), rnd(rh), rnd(rw), batch, heads, gh, gw, dh, dh ** -0.5)
        need = float((lg[..., :-1].max(-1).values - lg[..., -1]).max()) + margin + 1.0          # (+ 1: the rounding of hi + lo operands)
        v[:, -1, 1, :, 0] = 8.0 * np.ceil(need / (8.0 * dh ** -0.5) / 8.0)                  # the boost enters as scale * 8 * k
    elif regime == "bias_only":
        qkv[:, d:2 * d] = 0.0
    elif regime == "tables_zero":
        rh[:], rw[:] = 0.0, 0.0
    elif regime != "peaked":
        raise ValueError(regime)
    return qkv, rh, rw


def one_hot_operands(batch, heads, gh, gw, dh, dy, dx):
    """A structural probe that does not rest on the shifted-table identity: q = 40 e_0 for every query, k = 0, Rh zero except
    Rh[gh - 1 + dy][0] = 1, Rw likewise at gw - 1 + dx.  The logit of key (ky, kx) for query (y, x) is 40 [y - ky == dy] + 40 [x - kx == dx]:
    the key (y - dy, x - dx) leads every other by 40 (e^-40 = 4e-18).  v carries the key's position in channels 0 and 1 as
    ((ky + 1) / 64, (kx + 1) / 64) -- exact in bf16, at most 1, and never 0: an output channel whose leading key holds 0 would show the
    4e-18 terms of the others -- and (j % 7 + 1) / 8 in channel 2; the rest is 0.  Returns (qkv, rel_h, rel_w, src [N] int64: the key each query must return, -1 where
    (y - dy, x - dx) lies outside the grid)."""
    n, d = gh * gw, heads * dh
    qkv = np.zeros((batch, n, 3, heads, dh), np.float32)
    qkv[:, :, 0, :, 0] = 40.0
    ys, xs = np.divmod(np.arange(n), gw)
    qkv[:, :, 2, :, 0], qkv[:, :, 2, :, 1], qkv[:, :, 2, :, 2] = ((ys + 1) / 64)[None, :, None], ((xs + 1) / 64)[None, :, None], ((np.arange(n) % 7 + 1) / 8)[None, :, None]
    rh, rw = np.zeros((2 * gh - 1, dh), np.float32), np.zeros((2 * gw - 1, dh), np.float32)
    rh[gh - 1 + dy, 0] = 1.0
    rw[gw - 1 + dx, 0] = 1.0
    ky, kx = ys - dy, xs - dx
    src = np.where((ky >= 0) & (ky < gh) & (kx >= 0) & (kx < gw), ky * gw + kx, -1)
    return qkv.reshape(batch * n, 3 * d), rh, rw, src


# --------------------------------------------------------------------------------------------------------------------------------
# single modules (tests/test_gpu_vision_tower_modules.py): d = 128, 2 heads, seeded like the cases
# --------------------------------------------------------------------------------------------------------------------------------
MOD_D, MOD_HEADS = 128, 2
# per-kernel bounds of the suite for hi + lo operands, relative to max(1, max|ref|): a GEMM or an attention 2e-4 (test_gpu_kernel_routes.py),
# a conv 2e-4 (test_gpu_conv2d.py); a LayerNorm over d <= 256 with |y| <= 8 by norm_bound of test_gpu_head_kernels.py:
# (d / 64 + 8) u (max|y| + max|x| rstd max|gamma|) + 4 u |y| < 12 * 6e-8 * 24 + 2e-6 < 2e-5
K_GEMM = K_ATTN = K_CONV = 2e-4
K_LN = 2e-5
BLOCK_BOUND = 2 * K_LN + 3 * K_GEMM + K_ATTN + K_GEMM           # norm1, qkv, attention, proj, norm2, lin1, lin2
# name -> (batch, gh, gw, window_size, weight seed, input seed)
BLOCK_CASES = {
    "global_5x7": (2, 5, 7, 0, 51, 151),
    "win4_5x7": (2, 5, 7, 4, 52, 152),           # pads 3 rows and 1 column
    "win14_5x7": (2, 5, 7, 14, 53, 153),         # one window larger than the grid
    "win14_20x20": (1, 20, 20, 14, 54, 154),     # 2 x 2 windows, 8 pad rows and columns
}
PADDED_BLOCK_CASES = [n for n, c in BLOCK_CASES.items() if c[3] > 0]


def seeded_state(shapes, seed):
    """{key: seeded array} for (key, shape) pairs, e.g. of a module's state_dict()."""
    return {k: seeded(k, tuple(s), seed) for k, s in shapes}


def block_shapes(d, heads, table_h, table_w, mlp_ratio=4.0):
    hidden = int(d * mlp_ratio)
    return [("norm1.weight", (d,)), ("norm1.bias", (d,)), ("attn.rel_pos_h", (table_h, d // heads)), ("attn.rel_pos_w", (table_w, d // heads)),
            ("attn.qkv.weight", (3 * d, d)), ("attn.qkv.bias", (3 * d,)), ("attn.proj.weight", (d, d)), ("attn.proj.bias", (d,)),
            ("norm2.weight", (d,)), ("norm2.bias", (d,)), ("mlp.lin1.weight", (hidden, d)), ("mlp.lin1.bias", (hidden,)),
            ("mlp.lin2.weight", (d, hidden)), ("mlp.lin2.bias", (d,))]


@functools.lru_cache(maxsize=None)
def block_case(name):
    """(state, x [B, gh, gw, d] fp32) of a Block(dim=MOD_D, num_heads=MOD_HEADS, window_size, input_size=(gh, gw))."""
    b, gh, gw, ws, seed, xseed = BLOCK_CASES[name]
    sh, sw = (ws, ws) if ws > 0 else (gh, gw)
    return seeded_state(block_shapes(MOD_D, MOD_HEADS, 2 * sh - 1, 2 * sw - 1), seed), synth.randn((b, gh, gw, MOD_D), xseed)


@functools.lru_cache(maxsize=None)
def block_ref(name, variant=None):
    sd, x = block_case(name)
    out = block(sd, "", _d(x), MOD_HEADS, BLOCK_CASES[name][3], variant).numpy()
    out.setflags(write=False)
    return out


def attention_module_ref(sd, x, heads):
    """Attention.forward on x [B, gh, gw, d]: qkv, the grid attention with the tables resized to the grid, proj."""
    b, gh, gw, d = x.shape
    dh = d // heads
    qkv = (_d(x).reshape(b, gh * gw, d) @ _d(sd["qkv.weight"]).t() + _d(sd["qkv.bias"])).view(b, gh * gw, 3, heads, dh)
    q, k, v = qkv.permute(2, 0, 3, 1, 4)
    o = grid_attention(q, k, v, resized_rel(sd["rel_pos_h"], gh), resized_rel(sd["rel_pos_w"], gw), gh, gw, dh ** -0.5)
    o = o.permute(0, 2, 1, 3).reshape(b, gh, gw, d)
    return (o @ _d(sd["proj.weight"]).t() + _d(sd["proj.bias"])).numpy()


def mlp_ref(sd, x):
    return (TF.gelu(_d(x) @ _d(sd["lin1.weight"]).t() + _d(sd["lin1.bias"])) @ _d(sd["lin2.weight"]).t() + _d(sd["lin2.bias"])).numpy()


def patch_embed_ref(sd, x, p=16):
    """[B, 3, H, W] -> [B, H // p, W // p, d]: the strided conv (it drops the remainder rows and columns itself)."""
    return TF.conv2d(_d(x), _d(sd["proj.weight"]), _d(sd["proj.bias"]), stride=p).permute(0, 2, 3, 1).numpy()


NO_POS = dict(SMALL, img_size=128, window_size=3)            # a 64 x 128 image: patch grid 4 x 8, windows of 3 pad it to 6 x 9
NO_POS_INPUT, NO_POS_SEEDS = (3, 3, 64, 128), (45, 145)


@functools.lru_cache(maxsize=None)
def no_pos_case():
    """(state without pos_embed, x, fp64 output) of ImageEncoderViT(**NO_POS, use_abs_pos=False): block 0 windowed, block 1 global with
    tables of 15 rows (rel_pos_h resized to 7 on the 4-row grid)."""
    sd = {k: v for k, v in state(NO_POS, NO_POS_SEEDS[0]).items() if k != "pos_embed"}
    x = synth.randn(NO_POS_INPUT, NO_POS_SEEDS[1])
    out = encoder(NO_POS, sd, x, "no_pos")
    out.setflags(write=False)
    return sd, x, out
