"""oracle/decoder_oracle.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Plain torch-CPU fp64 restatement of one decode step of a Qwen2-architecture decoder layer with a KV cache (what
lvq_qwen2_decode_step runs per layer, include/lvq.h "Decode-step runtime"): RMSNorm, packed q|k|v projection + bias, rotary
embedding at the new position, append to the cache, grouped-query attention over positions 0..pos, o_proj + residual, RMSNorm,
gate|up projection, SiLU(gate) * up, down projection + residual.

Weights use the packed layout of lvq_qwen2_layer: wqkv = [q_proj | k_proj | v_proj] rows, wgu = [gate_proj | up_proj] rows.
The rotary frequencies and angles are computed in fp32 as transformers' Qwen2RotaryEmbedding computes them
(inv_freq = 1 / theta ** (arange(0, dh, 2) / dh), angle = position * inv_freq); everything else is fp64.
Pinned against transformers' Qwen2DecoderLayer in float64 by tests/test_oracle_decoder.py.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

SD = Dict[str, torch.Tensor]


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w


def rope_angles(pos: torch.Tensor, dh: int, theta: float) -> torch.Tensor:
    """pos [...] integer positions -> angles [..., dh / 2] (fp32 arithmetic, returned as fp64)."""
    inv = 1.0 / (theta ** (torch.arange(0, dh, 2, dtype=torch.int64).to(torch.float32) / dh))
    return (pos.to(torch.float32)[..., None] * inv).double()


def rope(x: torch.Tensor, ang: torch.Tensor) -> torch.Tensor:
    """rotate-half rotary embedding of x [..., dh] at angles [..., dh / 2] (broadcast over the leading dims), in fp64."""
    h = x.shape[-1] // 2
    c, s = torch.cos(ang), torch.sin(ang)
    a, b = x[..., :h], x[..., h:]
    return torch.cat((a * c - b * s, b * c + a * s), dim=-1)


def silu(g: torch.Tensor) -> torch.Tensor:
    return g / (1.0 + torch.exp(-g))


def decode_layer(x: torch.Tensor, W: SD, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: int, n_heads: int, n_kv_heads: int,
                 eps: float, theta: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One new token per sequence at position `pos`.  x [B, d]; k_cache / v_cache [B, P, dkv]: the rotated keys and the values of
    the earlier positions this token attends to (P = pos for a full cache).  Returns (x_out [B, d], k_new [B, dkv] rotated,
    v_new [B, dkv])."""
    B, d = x.shape
    dh = d // n_heads
    dkv = dh * n_kv_heads
    inter = W["wgu"].shape[0] // 2
    h = rms_norm(x, W["ln1"], eps)
    qkv = h @ W["wqkv"].t() + W["bqkv"]
    ang = rope_angles(torch.tensor(pos), dh, theta)
    q = rope(qkv[:, :d].view(B, n_heads, dh), ang)
    k_new = rope(qkv[:, d:d + dkv].view(B, n_kv_heads, dh), ang).reshape(B, dkv)
    v_new = qkv[:, d + dkv:]
    keys = torch.cat((k_cache, k_new[:, None]), dim=1).view(B, -1, n_kv_heads, dh)
    vals = torch.cat((v_cache, v_new[:, None]), dim=1).view(B, -1, n_kv_heads, dh)
    grp = torch.arange(n_heads) // (n_heads // n_kv_heads)                    # query head -> its key/value head
    keys, vals = keys[:, :, grp].transpose(1, 2), vals[:, :, grp].transpose(1, 2)     # [B, H, P + 1, dh]
    p = torch.softmax(torch.einsum("bhe,bhje->bhj", q, keys) / dh ** 0.5, dim=-1)
    o = torch.einsum("bhj,bhje->bhe", p, vals).reshape(B, d)
    x = x + o @ W["wo"].t()
    gu = rms_norm(x, W["ln2"], eps) @ W["wgu"].t()
    x = x + (silu(gu[:, :inter]) * gu[:, inter:]) @ W["wdown"].t()
    return x, k_new, v_new
