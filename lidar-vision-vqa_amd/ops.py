"""Thin Python wrappers over the fusion-side C ABI (include/lvq.h): argument marshalling only.

A "BF" value is a pair (hi, lo) of torch.bfloat16 tensors; lo is None for a plain-bf16 operand and the
residual x - hi for a split one (see include/lvq.h "Precision modes").  Modes:
  bf16    every operand plain (2^-9 operand rounding; fastest, ~3.5e-2 from the fp32 CPU reference on the bench workload)
  bf16x3  every operand hi + lo, every product hi*hi + hi*lo + lo*hi (meets the 1e-3 bar everywhere; 2.7x slower)
  mixed   bf16x3 everywhere EXCEPT the tensors whose rounding is independent per key of a long K/V stream and therefore
          averages out in the softmax-weighted sum (BEV tokens x, K, V, P of VATLiDAR's cross-attention: 262 144 keys): those
          stay plain.  Operands whose rounding is COMMON to all keys stay split: weights (W_proj, W_k|W_v), the conv tokens
          (93 % of the cells hold the same constant) and the query side.  tools/precision_study.py measures each group.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Tuple

import torch

from . import _ffi as F

BF = Tuple[torch.Tensor, Optional[torch.Tensor]]

PRECISIONS = ("bf16", "bf16x3", "mixed", "mixed16")
_default_precision = os.environ.get("LVQ_PRECISION", "bf16x3")
assert _default_precision in PRECISIONS


def default_precision() -> str:
    return _default_precision


def set_default_precision(p: str):
    global _default_precision
    if p not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}")
    _default_precision = p


# Optional per-launch timing with HIP events ON THE LAUNCH STREAM (bench.py's roofline leg): when EVENTS is a
# dict, every tagged launch appends (start, end) torch.cuda.Event pairs under its tag.
EVENTS = None


class _Region:
    def __init__(self, tag, device):
        self.tag, self.device = tag, device

    def __enter__(self):
        if EVENTS is not None and self.tag:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record(torch.cuda.current_stream(self.device))
        return self

    def __exit__(self, *exc):
        if EVENTS is not None and self.tag:
            self.e.record(torch.cuda.current_stream(self.device))
            EVENTS.setdefault(self.tag, []).append((self.s, self.e))
        return False


def region(tag, device):
    return _Region(tag, device)


def _bf_empty(shape, dev, split: bool) -> BF:
    hi = torch.empty(shape, dtype=torch.bfloat16, device=dev)
    return hi, (torch.empty(shape, dtype=torch.bfloat16, device=dev) if split else None)


def cast(x: torch.Tensor, split: bool) -> BF:
    F.require_cuda(x)
    assert x.dtype == torch.float32
    hi, lo = _bf_empty(x.shape, x.device, split)
    F.check(F.lib().lvq_cast_bf16(F.ptr(x), x.numel(), F.ptr(hi), F.ptr(lo), F.stream_ptr(x.device)), "lvq_cast_bf16")
    return hi, lo


def conv2d_pack_weights(weight: torch.Tensor, c_out: int, c_in: int, k: int, transposed: bool, split: bool) -> BF:
    """fp32 conv weights [c_out, c_in, k, k] (transposed: [c_in, c_out, k, k]) -> the packed bf16 (hi, lo) operand of lvq_conv2d /
    lvq_deconv2d (once per weights version)."""
    F.require_cuda(weight)
    L = F.lib()
    n = L.lvq_conv2d_packed_elems(c_out, c_in, k, int(transposed))
    if n == 0:
        raise F.LvqError(f"lvq_conv2d: {'ConvTranspose2d' if transposed else 'Conv2d'}({c_in} -> {c_out}, kernel {k}) is outside the kernel family")
    hi, lo = _bf_empty((n,), weight.device, split)
    F.check(L.lvq_conv2d_pack_weights(F.ptr(weight), c_out, c_in, k, int(transposed), F.ptr(hi), F.ptr(lo), F.stream_ptr(weight.device)),
            "lvq_conv2d_pack_weights")
    return hi, lo


def to_f32(x: BF, alpha: float = 1.0) -> torch.Tensor:
    hi, lo = x
    out = torch.empty(hi.shape, dtype=torch.float32, device=hi.device)
    F.check(F.lib().lvq_bf16_to_f32(F.ptr(hi), F.ptr(lo), hi.numel(), alpha, F.ptr(out),
                                    F.stream_ptr(hi.device)), "lvq_bf16_to_f32")
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: Optional[torch.Tensor], eps: float, split: bool,
              want_f32: bool = False, want_bf: bool = True, add: Optional[torch.Tensor] = None, add_group: int = 1,
              post: Optional[torch.Tensor] = None):
    """x [rows, d] fp32 -> (y_f32 | None, BF | None)."""
    F.require_cuda(x, gamma, beta, add, post)
    rows, d = x.shape
    y32 = torch.empty_like(x) if want_f32 else None
    hi, lo = _bf_empty(x.shape, x.device, split) if want_bf else (None, None)
    rc = F.lib().lvq_layernorm(F.ptr(x), F.ptr(add), add.shape[0] if add is not None else 0, add_group,
                               F.ptr(gamma), F.ptr(beta), eps, rows, d, F.ptr(post),
                               post.shape[0] if post is not None else 0, F.ptr(y32), F.ptr(hi), F.ptr(lo),
                               F.stream_ptr(x.device))
    F.check(rc, "lvq_layernorm")
    return y32, ((hi, lo) if want_bf else None)


def rmsnorm(x: torch.Tensor, gamma: torch.Tensor, eps: float, split: bool) -> BF:
    rows, d = x.shape
    hi, lo = _bf_empty(x.shape, x.device, split)
    rc = F.lib().lvq_rmsnorm(F.ptr(x), F.ptr(gamma), eps, rows, d, F.ptr(None), F.ptr(hi), F.ptr(lo),
                             F.stream_ptr(x.device))
    F.check(rc, "lvq_rmsnorm")
    return hi, lo


GEMM_GELU, GEMM_QUICK_GELU = 1, 2          # include/lvq.h: LVQ_GEMM_GELU, LVQ_GEMM_QUICK_GELU


def linear(a: BF, w: BF, bias: Optional[torch.Tensor] = None, *, gelu: bool = False, quick_gelu: bool = False, alpha: float = 1.0,
           residual: Optional[torch.Tensor] = None, rowtab: Optional[torch.Tensor] = None, out_f32: bool = False,
           out_bf: bool = False, w_rows: Optional[Tuple[int, int]] = None, w_cols: Optional[Tuple[int, int]] = None,
           a_rows: Optional[Tuple[int, int, int, int]] = None, tag: Optional[str] = None):
    """y = a @ w[r0:r1, c0:c1].T (+bias[r0:r1]) ... ; a hi [M, K], w hi [N, Kw] with K = c1 - c0 (the column slice is read through
    ldw = Kw, no copy).  a_rows = (batch, stride, first, m): rows first .. first + m - 1 of every `stride` rows of a, `batch` times
    (one batched launch; the rows between are skipped by the batch stride) -> y [batch * m, N].  gelu / quick_gelu: the epilogue's
    activation (exact erf / x sigmoid(1.702 x)).  Returns (y_f32 | None, BF | None)."""
    ah, al = a
    wh, wl = w
    kw = wh.shape[1]
    r0, r1 = w_rows if w_rows is not None else (0, wh.shape[0])
    c0, c1 = w_cols if w_cols is not None else (0, kw)
    n, k = r1 - r0, c1 - c0
    batch, a_bs, first, m = (1, 0, 0, ah.shape[0]) if a_rows is None else (a_rows[0], a_rows[1] * k, a_rows[2], a_rows[3])
    assert ah.shape[1] == k and (al is None or wl is not None)      # plain | bf16x3 | a plain, w split ("x2w")
    assert (first + m) + (batch - 1) * (a_bs // k) <= ah.shape[0] and c0 % 8 == 0
    dev = ah.device
    split = wl is not None
    rows = batch * m
    c32 = torch.empty((rows, n), dtype=torch.float32, device=dev) if out_f32 else None
    ch, cl = _bf_empty((rows, n), dev, al is not None) if out_bf else (None, None)
    wo = (r0 * kw + c0) * 2  # byte offset of the weight slice
    ao = first * k * 2
    bo = r0 * 4
    with region(tag, dev):
        rc = F.lib().lvq_gemm_bf16(
            ah.data_ptr() + ao, al.data_ptr() + ao if al is not None else None, wh.data_ptr() + wo, wl.data_ptr() + wo if split else None,
            bias.data_ptr() + bo if bias is not None else None, F.ptr(residual), F.ptr(rowtab),
            rowtab.shape[0] if rowtab is not None else 0, alpha, (GEMM_GELU if gelu else 0) | (GEMM_QUICK_GELU if quick_gelu else 0), m, n,
            k, k, kw, n, batch, a_bs, 0, 0 if a_rows is None else m * n, F.ptr(c32), F.ptr(ch), F.ptr(cl),
            F.stream_ptr(dev))
    F.check(rc, f"lvq_gemm_bf16 (m={m}, n={n}, k={k}, batch={batch})")
    return c32, ((ch, cl) if out_bf else None)


def clip_embed_ok(batch: int, c: int, hw: int) -> bool:
    """lvq_clip_embed_ok: the embedding kernel takes (batch, c, hw)."""
    return bool(F.lib().lvq_clip_embed_ok(batch, c, hw))


def clip_embed(feat: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, gamma: torch.Tensor, beta: Optional[torch.Tensor], eps: float,
               *, want_tok: bool = False, split: bool = False, tag: Optional[str] = None):
    """lvq_clip_embed.  feat [B, c, hw] fp32 channel-major, cls [c], pos [1 + hw, c] -> (hidden [B * (1 + hw), c] fp32,
    tok BF [B * hw, c] | None): LayerNorm(cat(cls, feat^T) + pos), and feat^T as a GEMM operand (hi, lo with `split`)."""
    F.require_cuda(feat, cls, pos, gamma, beta)
    if feat.dim() != 3 or feat.dtype != torch.float32:
        raise F.LvqError(f"clip_embed: feat must be fp32 [batch, c, hw], got {feat.dtype} {tuple(feat.shape)}")
    b, c, hw = feat.shape
    if tuple(cls.shape) != (c,) or tuple(pos.shape) != (1 + hw, c) or tuple(gamma.shape) != (c,):
        raise F.LvqError(f"clip_embed: cls {tuple(cls.shape)}, pos {tuple(pos.shape)}, gamma {tuple(gamma.shape)} do not fit feat {tuple(feat.shape)}")
    hidden = torch.empty((b * (1 + hw), c), dtype=torch.float32, device=feat.device)
    th, tl = _bf_empty((b * hw, c), feat.device, split) if want_tok else (None, None)
    with region(tag, feat.device):
        rc = F.lib().lvq_clip_embed(F.ptr(feat), F.ptr(cls), F.ptr(pos), F.ptr(gamma), F.ptr(beta), eps, b, c, hw, F.ptr(hidden),
                                    F.ptr(th), F.ptr(tl), c, F.stream_ptr(feat.device))
    F.check(rc, f"lvq_clip_embed (batch={b}, c={c}, hw={hw})")
    return hidden, ((th, tl) if want_tok else None)


def attention(q: BF, k: BF, v: BF, *, batch: int, n_heads: int, n_kv_heads: int, nq: int, nkv: int, dh: int,
              q_strides, k_strides, v_strides, scale: float, bias: Optional[torch.Tensor] = None, causal: bool = False,
              tag: Optional[str] = None) -> BF:
    """q/k/v: BF views (possibly column slices of packed projections); *_strides = (batch, row, head) in elements.
    Returns BF [batch*nq, n_heads*dh]."""
    qh, ql = q
    dev = qh.device
    split = ql is not None                       # q split, k / v plain = the "mixed" stream form (lvq_attention_stream_ok shapes)
    oh, ol = _bf_empty((batch * nq, n_heads * dh), dev, split)
    L = F.lib()
    nbytes = L.lvq_attention_workspace_bytes(batch, n_heads, nq, nkv, dh,
                                             3 if k[1] is not None else 1)
    ws = F.workspace(nbytes, dev, "attn")
    d = n_heads * dh
    with region(tag, dev):
        rc = L.lvq_attention_bf16(
            F.ptr(qh), F.ptr(ql), F.ptr(k[0]), F.ptr(k[1]), F.ptr(v[0]), F.ptr(v[1]), F.ptr(bias), batch, n_heads,
            n_kv_heads, nq, nkv, dh,
            q_strides[0], q_strides[1], q_strides[2],
            k_strides[0], k_strides[1], k_strides[2],
            v_strides[0], v_strides[1], v_strides[2],
            nq * d, d, dh, scale, 1 if causal else 0, F.ptr(oh), F.ptr(ol),
            F.ptr(ws), ws.numel(), F.stream_ptr(dev))
    F.check(rc, f"lvq_attention_bf16 (B={batch}, H={n_heads}, nq={nq}, nkv={nkv}, dh={dh})")
    return oh, ol


def attention_relpos_ok(gh: int, gw: int, dh: int) -> bool:
    """lvq_attention_relpos_ok: the fused grid attention with decomposed relative-position bias takes (gh, gw, dh)."""
    return bool(F.lib().lvq_attention_relpos_ok(gh, gw, dh))


def attention_relpos(qkv: BF, rel_h: BF, rel_w: BF, *, batch: int, n_heads: int, gh: int, gw: int, dh: int, scale: float,
                     tag: Optional[str] = None) -> BF:
    """lvq_attention_relpos_bf16.  qkv: BF [batch * gh * gw, >= 3 * n_heads * dh] (the packed projection, row stride = its width);
    rel_h [2 gh - 1, dh], rel_w [2 gw - 1, dh].  Returns BF [batch * gh * gw, n_heads * dh]."""
    qh, ql = qkv
    dev = qh.device
    split = ql is not None
    F.require_cuda(qh, ql, rel_h[0], rel_h[1], rel_w[0], rel_w[1])
    if qh.dim() != 2 or qh.shape[0] != batch * gh * gw or tuple(rel_h[0].shape) != (2 * gh - 1, dh) or tuple(rel_w[0].shape) != (2 * gw - 1, dh):
        raise F.LvqError(f"attention_relpos: qkv {tuple(qh.shape)}, rel_h {tuple(rel_h[0].shape)}, rel_w {tuple(rel_w[0].shape)} do not "
                         f"fit batch {batch}, grid {gh} x {gw}, head dim {dh}")
    oh, ol = _bf_empty((batch * gh * gw, n_heads * dh), dev, split)
    L = F.lib()
    nbytes = L.lvq_attention_relpos_workspace_bytes(batch, n_heads, gh, gw, dh, 3 if split else 1)
    ws = F.workspace(nbytes, dev, "attn") if nbytes else None
    with region(tag, dev):
        rc = L.lvq_attention_relpos_bf16(F.ptr(qh), F.ptr(ql), qh.shape[1], F.ptr(rel_h[0]), F.ptr(rel_h[1]), F.ptr(rel_w[0]),
                                         F.ptr(rel_w[1]), batch, n_heads, gh, gw, dh, scale,
                                         F.ptr(oh), F.ptr(ol), n_heads * dh, F.ptr(ws), ws.numel() if ws is not None else 0,
                                         F.stream_ptr(dev))
    F.check(rc, f"lvq_attention_relpos_bf16 (B={batch}, H={n_heads}, grid {gh} x {gw}, dh={dh})")
    return oh, ol


def attention_decode_ragged(q: BF, k_cache: BF, v_cache: BF, kv_len: torch.Tensor, *, batch: int, n_heads: int, n_kv_heads: int, lmax: int,
                            dh: int, q_strides, k_strides, v_strides, scale: float) -> BF:
    """One query token per sequence over the first kv_len[b] rows of its K / V cache (include/lvq.h: lvq_attention_decode_ragged).
    q / k_cache / v_cache: BF views, *_strides = (batch, row, head) in elements as in `attention`; kv_len: int32 [batch] on the
    device.  Returns BF [batch, n_heads*dh] (lo part when q is split)."""
    qh, ql = q
    dev = qh.device
    if kv_len.dtype != torch.int32 or kv_len.device != dev or kv_len.numel() != batch or not kv_len.is_contiguous():
        raise F.LvqError("attention_decode_ragged: kv_len must be a contiguous int32 tensor [batch] on the operands' device")
    split = ql is not None
    oh, ol = _bf_empty((batch, n_heads * dh), dev, split)
    L = F.lib()
    nbytes = L.lvq_attention_decode_ragged_workspace_bytes(batch, n_heads, n_kv_heads, lmax, dh,
                                                           3 if split else 1)
    ws = F.workspace(nbytes, dev, "attn_ragged")
    d = n_heads * dh
    rc = L.lvq_attention_decode_ragged(
        F.ptr(qh), F.ptr(ql), F.ptr(k_cache[0]), F.ptr(k_cache[1]), F.ptr(v_cache[0]), F.ptr(v_cache[1]), F.ptr(kv_len), batch,
        n_heads, n_kv_heads, lmax, dh,
        q_strides[0], q_strides[1], q_strides[2],
        k_strides[0], k_strides[1], k_strides[2],
        v_strides[0], v_strides[1], v_strides[2],
        d, d, dh, scale, F.ptr(oh), F.ptr(ol), F.ptr(ws), ws.numel(), F.stream_ptr(dev))
    F.check(rc, f"lvq_attention_decode_ragged (B={batch}, H={n_heads}, Hkv={n_kv_heads}, lmax={lmax}, dh={dh})")
    return oh, ol


def attention_extend_shared(q: BF, pk_cache: BF, pv_cache: BF, k_cache: BF, v_cache: BF, prefix_index: torch.Tensor, plen: torch.Tensor,
                            own0: torch.Tensor, qn: torch.Tensor, *, n_heads: int, n_kv_heads: int, dh: int, scale: float) -> BF:
    """Ragged chunks of query rows behind shared prefixes (include/lvq.h: lvq_attention_extend_shared).  q: BF [batch, lq, n_heads*dh];
    prefix caches BF [n_prefix, pmax, n_kv_heads*dh]; own caches BF [batch, lown, n_kv_heads*dh] (they already hold the keys / values of
    the query rows at own0[b] .. own0[b] + qn[b] - 1); prefix_index / own0 / qn: int32 [batch], plen: int32 [n_prefix], all on the device.
    Every tensor contiguous.  Returns BF [batch, lq, n_heads*dh] (lo part when q is split)."""
    qh, ql = q
    dev = qh.device
    batch, lq, d = qh.shape
    n_prefix, pmax, dkv = pk_cache[0].shape
    lown = k_cache[0].shape[1]
    if d != n_heads * dh or dkv != n_kv_heads * dh or tuple(k_cache[0].shape) != (batch, lown, dkv):
        raise F.LvqError("attention_extend_shared: q [batch, lq, H*dh], prefix caches [G, pmax, Hkv*dh], own caches [batch, lown, Hkv*dh]")
    for name, t, n in (("prefix_index", prefix_index, batch), ("plen", plen, n_prefix), ("own0", own0, batch), ("qn", qn, batch)):
        if t.dtype != torch.int32 or t.device != dev or t.numel() != n or not t.is_contiguous():
            raise F.LvqError(f"attention_extend_shared: {name} must be a contiguous int32 tensor [{n}] on the operands' device")
    split = ql is not None
    F.require_cuda(qh, ql, *pk_cache, *pv_cache, *k_cache, *v_cache)
    oh, ol = _bf_empty((batch, lq, d), dev, split)
    L = F.lib()
    nbytes = L.lvq_attention_extend_shared_workspace_bytes(batch, lq, n_heads, n_kv_heads, pmax,
                                                           lown, dh, 3 if split else 1)
    ws = F.workspace(nbytes, dev, "attn_shared")
    rc = L.lvq_attention_extend_shared(
        F.ptr(qh), F.ptr(ql), F.ptr(pk_cache[0]), F.ptr(pk_cache[1]), F.ptr(pv_cache[0]), F.ptr(pv_cache[1]), F.ptr(k_cache[0]),
        F.ptr(k_cache[1]), F.ptr(v_cache[0]), F.ptr(v_cache[1]), F.ptr(prefix_index), F.ptr(plen), F.ptr(own0), F.ptr(qn), batch,
        lq, n_heads, n_kv_heads, n_prefix, pmax, lown, dh,
        lq * d, d, dh, pmax * dkv, lown * dkv, dkv, dh,
        pmax * dkv, lown * dkv, dkv, dh, lq * d, d, dh, scale, F.ptr(oh), F.ptr(ol),
        F.ptr(ws), ws.numel(), F.stream_ptr(dev))
    F.check(rc, f"lvq_attention_extend_shared (B={batch}, lq={lq}, H={n_heads}, Hkv={n_kv_heads}, G={n_prefix}, pmax={pmax}, lown={lown}, dh={dh})")
    return oh, ol


def ca_fused_ok(batch: int, nq: int, nkv: int, d: int, n_heads: int) -> bool:
    """Shapes of the fused short-K/V cross-attention kernel (include/lvq.h: lvq_ca_fused_ok)."""
    return bool(F.lib().lvq_ca_fused_ok(batch, nq, nkv, d, n_heads))


def ca_fused_pack(ln_w: torch.Tensor, ln_b: torch.Tensor, in_w: torch.Tensor, in_b: torch.Tensor, out_w: torch.Tensor, out_b: torch.Tensor,
                  n_heads: int, f16: bool) -> torch.Tensor:
    """ca_ln + ca weights -> the fragment-major 16-bit blob of lvq_ca_fused (once per weights version)."""
    F.require_cuda(ln_w, ln_b, in_w, in_b, out_w, out_b)
    d = out_w.shape[0]
    L = F.lib()
    nbytes = int(L.lvq_ca_fused_packed_bytes(d, n_heads))
    if nbytes == 0:
        raise F.LvqError(f"lvq_ca_fused: d={d}, heads={n_heads} is not a shape of the fused kernel")
    blob = torch.empty(nbytes, dtype=torch.uint8, device=out_w.device)
    rc = L.lvq_ca_fused_pack(F.ptr(ln_w), F.ptr(ln_b), F.ptr(in_w), F.ptr(in_b), F.ptr(out_w), F.ptr(out_b), d, n_heads,
                             1 if f16 else 0, F.ptr(blob), nbytes, F.stream_ptr(out_w.device))
    F.check(rc, "lvq_ca_fused_pack")
    return blob


def ca_fused(q: torch.Tensor, kv: torch.Tensor, blob: torch.Tensor, eps: float, n_heads: int, f16: bool, tag: Optional[str] = None) -> torch.Tensor:
    """out = q + ca(ca_ln(q), kv, kv) for q [B, nq, d], kv [B, nkv, d] fp32 (vat_blocks.py:41-42) in two launches."""
    F.require_cuda(q, kv, blob)
    B, nq, d = q.shape
    nkv = kv.shape[1]
    dev = q.device
    L = F.lib()
    nbytes = int(L.lvq_ca_fused_workspace_bytes(B, nq, nkv, d, n_heads))
    if nbytes == 0:
        raise F.LvqError(f"lvq_ca_fused: (B={B}, nq={nq}, nkv={nkv}, d={d}, heads={n_heads}) is not a shape of the fused kernel")
    ws = F.workspace(nbytes, dev, "ca_fused")
    out = torch.empty_like(q)
    with region(tag, dev):
        rc = L.lvq_ca_fused(F.ptr(q), F.ptr(kv), F.ptr(blob), eps, B, nq, nkv, d, n_heads,
                            1 if f16 else 0, F.ptr(out), F.ptr(ws), ws.numel(), F.stream_ptr(dev))
    F.check(rc, f"lvq_ca_fused (B={B}, nq={nq}, nkv={nkv})")
    return out


def attention_stream_ok(nq: int, nkv: int, dh: int) -> bool:
    """True when lvq_attention_bf16 takes (q split, k / v plain) for this shape: the long-stream kernel's shapes."""
    return bool(F.lib().lvq_attention_stream_ok(nq, nkv, dh))


def bev_occupied_cells(bev: torch.Tensor, cap: Optional[int] = None):
    """Dense canvas [B, C, H, W] fp32 -> its occupied cells as pillars: feats [cap, C] fp32, coords [cap, 4] int32 (b, 0, y, x), n [1] int32 on the
    device (rows >= n are not written; cap defaults to every cell).  lvq_bev_occupied_cells: the inverse of PointPillarScatter."""
    F.require_cuda(bev)
    B, C, H, W = bev.shape
    cap = B * H * W if cap is None else int(cap)
    feats = torch.empty((cap, C), dtype=torch.float32, device=bev.device)
    coords = torch.empty((cap, 4), dtype=torch.int32, device=bev.device)
    n = torch.empty(1, dtype=torch.int32, device=bev.device)
    rc = F.lib().lvq_bev_occupied_cells(F.ptr(bev), B, C, H, W, cap, F.ptr(feats), F.ptr(coords), F.ptr(n),
                                        F.stream_ptr(bev.device))
    F.check(rc, "lvq_bev_occupied_cells")
    return feats, coords, n


def dwconv3x3_gelu(bev: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], split: bool) -> BF:
    """bev [B,C,H,W] fp32 -> tokens BF [B*H*W, C]."""
    F.require_cuda(bev, w, b)
    B, C, H, W = bev.shape
    hi, lo = _bf_empty((B * H * W, C), bev.device, split)
    rc = F.lib().lvq_dwconv3x3_gelu(F.ptr(bev), F.ptr(w), F.ptr(b), B, C, H, W, F.ptr(hi),
                                    F.ptr(lo), F.stream_ptr(bev.device))
    F.check(rc, "lvq_dwconv3x3_gelu")
    return hi, lo


def pillar_dwconv3x3_gelu(feat: torch.Tensor, coords: torch.Tensor, n_live: Optional[torch.Tensor], batch: int, ny: int, nx: int,
                          w: torch.Tensor, b: Optional[torch.Tensor], split: bool) -> BF:
    """Sparse BEV bridge: PointPillarScatter + depthwise 3x3 + GELU -> tokens BF [batch*ny*nx, C] without the dense canvas
    (bit-identical to pillar_scatter + dwconv3x3_gelu).  feat [M, C] fp32, coords [M, 4] int32 (b, z, y, x), rows >= n_live[0] skipped."""
    F.require_cuda(feat, coords, w, b, n_live)
    m, C = feat.shape
    hi, lo = _bf_empty((batch * ny * nx, C), feat.device, split)
    L = F.lib()
    nbytes = int(L.lvq_pillar_dwconv_workspace_bytes(batch, ny, nx))
    ws = F.workspace(nbytes, feat.device, "pillar_dwconv")
    rc = L.lvq_pillar_dwconv3x3_gelu(F.ptr(feat), F.ptr(coords), m, F.ptr(n_live), C, batch, ny, nx,
                                     F.ptr(w), F.ptr(b), F.ptr(hi), F.ptr(lo), F.ptr(ws), ws.numel(), F.stream_ptr(feat.device))
    F.check(rc, "lvq_pillar_dwconv3x3_gelu")
    return hi, lo


# ---- sparse (tiled) BEV key stream: include/lvq.h "sparse BEV key stream of VATLiDAR" ----
def pillar_index_map(coords: torch.Tensor, n_live: Optional[torch.Tensor], batch: int, ny: int, nx: int) -> torch.Tensor:
    """[batch, ny, nx] int32: pillar row or -1 (PointPillarScatter as an index map)."""
    F.require_cuda(coords, n_live)
    idx = torch.empty((batch, ny, nx), dtype=torch.int32, device=coords.device)
    rc = F.lib().lvq_pillar_index_map(F.ptr(coords), coords.shape[0], F.ptr(n_live), batch, ny, nx, F.ptr(idx),
                                      F.stream_ptr(coords.device))
    F.check(rc, "lvq_pillar_index_map")
    return idx


def bev_tiles(idx: Optional[torch.Tensor], batch: int, ny: int, nx: int, device, row_base: int, force_all: bool = False):
    """Piece / row bookkeeping of the tiled key stream (8 x 8-cell tiles of eight 2 x 4-cell pieces; a cell is dirty when its 3 x 3
    neighbourhood holds a pillar) -> (live_list [batch*nt*8] i32, piece_dirty [batch*nt*8, 2] i32, row_src [batch, ny*nx] i32 absolute rows
    of the K|V buffer (dirty: row_base + number, clean: table row = key index), counts [3] i32 = live pieces, their rows, dirty rows)."""
    nt = (ny // 8) * (nx // 8)
    live = torch.empty((batch * nt * 8,), dtype=torch.int32, device=device)
    dirty = torch.empty((batch * nt * 8, 2), dtype=torch.int32, device=device)
    src = torch.empty((batch, ny * nx), dtype=torch.int32, device=device)
    counts = torch.empty((3,), dtype=torch.int32, device=device)
    L = F.lib()
    nbytes = int(L.lvq_bev_tiles_workspace_bytes(batch, ny, nx))
    ws = F.workspace(nbytes, device, "bev_tiles", per_stream=True)
    rc = L.lvq_bev_tiles(F.ptr(idx), batch, ny, nx, 1 if force_all else 0, row_base, F.ptr(live), F.ptr(dirty),
                         F.ptr(src), F.ptr(counts), F.ptr(ws), ws.numel(), F.stream_ptr(device))
    F.check(rc, "lvq_bev_tiles")
    return live, dirty, src, counts


def bev_tile_tokens(feat: torch.Tensor, idx: torch.Tensor, live: torch.Tensor, dirty: torch.Tensor, counts: torch.Tensor, cap_rows: int, batch: int, ny: int, nx: int,
                    w9: torch.Tensor, b9: Optional[torch.Tensor], w: BF, bias, gamma, beta, eps: float, pe_tiled: torch.Tensor,
                    out_lo: bool, tag: Optional[str] = None) -> BF:
    """Fused refine conv -> proj -> LayerNorm -> + positional table over the live pieces; the DIRTY cells' rows are stored compactly
    -> x BF [cap_rows, n] (rows 0 .. counts[2]-1 written)."""
    F.require_cuda(feat, idx, live, dirty, counts, w9, b9, pe_tiled)
    n = w[0].shape[0]
    xh, xl = _bf_empty((cap_rows, n), feat.device, out_lo)
    with region(tag, feat.device):
        rc = F.lib().lvq_bev_tile_tokens(F.ptr(feat), F.ptr(idx), F.ptr(live), F.ptr(dirty), F.ptr(counts), batch * (ny // 8) * (nx // 8), batch,
                                         ny, nx, feat.shape[1], F.ptr(w9), F.ptr(b9), F.ptr(w[0]), F.ptr(w[1]), F.ptr(bias),
                                         F.ptr(gamma), F.ptr(beta), eps, F.ptr(pe_tiled), n, F.ptr(xh), F.ptr(xl),
                                         F.stream_ptr(feat.device))
    F.check(rc, "lvq_bev_tile_tokens")
    return xh, xl


def bev_tile_kv(feat: torch.Tensor, idx: torch.Tensor, live: torch.Tensor, dirty: torch.Tensor, counts: torch.Tensor, cap_rows: int, batch: int, ny: int,
                nx: int, w9: torch.Tensor, b9: Optional[torch.Tensor], m: BF, m0: torch.Tensor, r: BF, r0: torch.Tensor, c0: float, d_ln: int, eps: float,
                t_tiled: torch.Tensor, out: torch.Tensor, tag: Optional[str] = None, split_launch: bool = True, k_fp16: bool = False) -> torch.Tensor:
    """K|V rows of the dirty cells straight from the pillar features (lvq_bev_tile_kv: LayerNorm and the K|V projection folded onto the
    64-channel conv token) -> `out` [>= cap_rows, 2n] plain bf16, rows 0 .. counts[2]-1 written."""
    F.require_cuda(feat, idx, live, dirty, counts, w9, b9, m0, r0, t_tiled, out)
    n2 = m[0].shape[0]
    if out.dtype != torch.bfloat16 or not out.is_contiguous() or out.shape[0] < cap_rows or out.shape[1] != n2 or t_tiled.shape[1] != n2:
        raise F.LvqError("bev_tile_kv: `out` must be a contiguous bf16 [>= cap_rows, 2n] buffer and the table [HW, 2n]")
    t_f16 = t_tiled.dtype == torch.float16                       # fp16 table: two-launch form only
    if t_tiled.dtype not in (torch.float16, torch.float32) or (t_f16 and not split_launch):
        raise F.LvqError("bev_tile_kv: the table is fp32, or fp16 with the two-launch form")
    L = F.lib()
    cap_tiles = batch * (ny // 8) * (nx // 8)
    ws = None
    if split_launch:
        nbytes = int(L.lvq_bev_tile_kv_workspace_bytes(cap_tiles))
        ws = F.workspace(nbytes, feat.device, "tile_kv", per_stream=True)
    with region(tag, feat.device):
        rc = L.lvq_bev_tile_kv(F.ptr(feat), F.ptr(idx), F.ptr(live), F.ptr(dirty), F.ptr(counts), cap_tiles, batch,
                               ny, nx, feat.shape[1], F.ptr(w9), F.ptr(b9), F.ptr(m[0]), F.ptr(m[1]), F.ptr(m0), F.ptr(r[0]),
                               F.ptr(r[1]), F.ptr(r0), c0, d_ln, eps, F.ptr(t_tiled), 1 if t_f16 else 0, n2 // 2,
                               1 if k_fp16 else 0, F.ptr(out),
                               F.ptr(ws), ws.numel() if ws is not None else 0, F.stream_ptr(feat.device))
    F.check(rc, "lvq_bev_tile_kv")
    return out


def linear_live_rows(a: BF, w: BF, bias: Optional[torch.Tensor], rows_dev: torch.Tensor, w_rows, tag: Optional[str] = None,
                     out: Optional[torch.Tensor] = None) -> BF:
    """a [cap, k] @ w[r0:r1].T + bias over the first *rows_dev rows (device-side count) -> BF [cap, n] (hi only unless a is split).
    `out` (plain bf16 [>= cap, n], contiguous): write there instead of a fresh buffer."""
    ah, al = a
    wh, wl = w
    cap, k = ah.shape
    r0, r1 = w_rows
    n = r1 - r0
    if out is not None:
        if al is not None or out.dtype != torch.bfloat16 or not out.is_contiguous() or out.shape[0] < cap or out.shape[1] != n:
            raise F.LvqError("linear_live_rows: `out` must be a contiguous plain bf16 [>= cap, n] buffer")
        ch, cl = out, None
    else:
        ch, cl = _bf_empty((cap, n), ah.device, al is not None)
    wo, bo = r0 * k * 2, r0 * 4
    with region(tag, ah.device):
        rc = F.lib().lvq_gemm_bf16_live_rows(F.ptr(ah), F.ptr(al), wh.data_ptr() + wo,
                                             wl.data_ptr() + wo if wl is not None else None,
                                             bias.data_ptr() + bo if bias is not None else None, cap, F.ptr(rows_dev), n,
                                             k, k, k, n, F.ptr(ch), F.ptr(cl), F.stream_ptr(ah.device))
    F.check(rc, f"lvq_gemm_bf16_live_rows (cap={cap}, n={n}, k={k})")
    return ch, cl


def attention_tiled(q: BF, kv: torch.Tensor, row_src: torch.Tensor, *, batch: int, n_heads: int, nq: int, n_tiles: int, dh: int, scale: float,
                    tag: Optional[str] = None, k_fp16: bool = False) -> BF:
    """q BF [batch*nq, d]; kv [rows, 2d] plain bf16 (K | V packed): the per-model table rows and every batch's computed rows in ONE buffer;
    row_src [batch, n_tiles*64] i32 = the row of every key slot -> BF [batch*nq, d]."""
    qh, ql = q
    dev = qh.device
    d = n_heads * dh
    oh, ol = _bf_empty((batch * nq, d), dev, ql is not None)
    L = F.lib()
    nbytes = int(L.lvq_attention_workspace_bytes(batch, n_heads, nq, n_tiles * 64, dh, 1))
    ws = F.workspace(nbytes, dev, "attn")
    with region(tag, dev):
        rc = L.lvq_attention_bf16_tiled(F.ptr(qh), F.ptr(ql), F.ptr(kv), F.ptr(kv[:, d:]), F.ptr(row_src), batch, n_heads, nq,
                                        n_tiles, dh, nq * d, d, dh, 2 * d, dh, nq * d, d,
                                        dh, scale, 1 if k_fp16 else 0, F.ptr(oh), F.ptr(ol), F.ptr(ws), ws.numel(),
                                        F.stream_ptr(dev))
    F.check(rc, f"lvq_attention_bf16_tiled (B={batch}, H={n_heads}, nq={nq}, tiles={n_tiles})")
    return oh, ol


def attention_stream_totals(q: BF, kv: torch.Tensor, *, n_heads: int, nq: int, nkv: int, dh: int, scale: float, k_fp16: int = 0) -> torch.Tensor:
    """Unnormalised softmax sums (O | m | l) of ONE batch of queries q BF [nq, d] over the dense key stream kv [nkv, 2d] (K | V packed,
    plain bf16) -> fp32 [n_heads, nq, dh + 2]: the per-model totals of attention_tiled_signed."""
    qh, ql = q
    dev = qh.device
    d = n_heads * dh
    L = F.lib()
    nbytes = int(L.lvq_attention_stream_totals_workspace_bytes(n_heads, nq, nkv, dh))
    if nbytes == 0:
        raise F.LvqError(f"attention_stream_totals: shape (nq={nq}, nkv={nkv}, dh={dh}) is not a long-stream shape")
    ws = F.workspace(nbytes, dev, "attn")
    tot = torch.empty((n_heads, nq, dh + 2), dtype=torch.float32, device=dev)
    rc = L.lvq_attention_bf16_stream_totals(F.ptr(qh), F.ptr(ql), F.ptr(kv), F.ptr(kv[:, d:]), n_heads, nq, nkv, dh,
                                            d, dh, 2 * d, dh, scale, int(k_fp16), F.ptr(tot), F.ptr(ws), ws.numel(),
                                            F.stream_ptr(dev))
    F.check(rc, f"lvq_attention_bf16_stream_totals (H={n_heads}, nq={nq}, nkv={nkv})")
    return tot


def bev_scene_pairs(row_src: torch.Tensor, batch: int, n_tiles: int, row_base: int):
    """Per-scene pair lists of the signed stream -> (pair_src [batch, n_tiles, 64] i32, pair_info [batch, 2] i32 = pair tiles, use flag)."""
    dev = row_src.device
    pair_src = torch.empty((batch, n_tiles, 64), dtype=torch.int32, device=dev)
    pair_info = torch.empty((batch, 2), dtype=torch.int32, device=dev)
    rc = F.lib().lvq_bev_scene_pairs(F.ptr(row_src), batch, n_tiles, row_base, n_tiles, F.ptr(pair_src),
                                     F.ptr(pair_info), F.stream_ptr(dev))
    F.check(rc, "lvq_bev_scene_pairs")
    return pair_src, pair_info


def attention_tiled_signed(q: BF, kv: torch.Tensor, row_src: torch.Tensor, pair_src: torch.Tensor, pair_info: torch.Tensor, totals: torch.Tensor, *, batch: int, n_heads: int, nq: int, n_tiles: int, dh: int, scale: float,
                           shared_q: bool, tag: Optional[str] = None, k_fp16: bool = False, stats: Optional[torch.Tensor] = None) -> BF:
    """attention_tiled over the dirty rows only (queries independent of the batch; `totals` from attention_stream_totals with the
    SAME q over the table rows kv[:n_tiles*64]).  q BF [nq, d] when shared_q else [batch*nq, d] (identical per batch) -> BF [batch*nq, d]."""
    qh, ql = q
    dev = qh.device
    d = n_heads * dh
    oh, ol = _bf_empty((batch * nq, d), dev, ql is not None)
    L = F.lib()
    nbytes = int(L.lvq_attention_tiled_signed_workspace_bytes(batch, n_heads, nq, n_tiles, dh))
    if nbytes == 0:
        raise F.LvqError(f"attention_tiled_signed: shape (nq={nq}, tiles={n_tiles}, dh={dh}) is not a long-stream shape")
    ws = F.workspace(nbytes, dev, "attn")
    with region(tag, dev):
        rc = L.lvq_attention_bf16_tiled_signed(F.ptr(qh), F.ptr(ql), F.ptr(kv), F.ptr(kv[:, d:]), F.ptr(row_src), F.ptr(pair_src), F.ptr(pair_info), pair_src.shape[1], F.ptr(totals),
                                               batch, n_heads, nq, n_tiles, dh,
                                               0 if shared_q else nq * d, d, dh, 2 * d, dh, nq * d, d,
                                               dh, scale, 1 if k_fp16 else 0, F.ptr(oh), F.ptr(ol), F.ptr(stats), F.ptr(ws), ws.numel(), F.stream_ptr(dev))
    F.check(rc, f"lvq_attention_bf16_tiled_signed (B={batch}, H={n_heads}, nq={nq}, tiles={n_tiles})")
    return oh, ol


def bev_shared_lists(row_src: torch.Tensor, batch: int, n_tiles: int, row_base: int):
    """Lists of the shared subtraction (include/lvq.h: lvq_bev_shared_lists) -> (list_src [batch + 1, n_tiles, 64] i32, list_info
    [batch + 1, 4] i32 = tiles, use flag, first add tile, first ignore tile); entry `batch` is the list of the shared set G."""
    dev = row_src.device
    L = F.lib()
    list_src = torch.empty((batch + 1, n_tiles, 64), dtype=torch.int32, device=dev)
    list_info = torch.empty((batch + 1, 4), dtype=torch.int32, device=dev)
    ws = F.workspace(64 * n_tiles + 512 * (batch + 1) + 512, dev, "shared_lists")      # include/lvq.h: lvq_bev_shared_lists
    rc = L.lvq_bev_shared_lists(F.ptr(row_src), batch, n_tiles, row_base, n_tiles, F.ptr(list_src), F.ptr(list_info), F.ptr(ws), ws.numel(),
                                F.stream_ptr(dev))
    F.check(rc, "lvq_bev_shared_lists")
    return list_src, list_info


def attention_tiled_shared(q: BF, kv: torch.Tensor, row_src: torch.Tensor, list_src: torch.Tensor, list_info: torch.Tensor, totals: torch.Tensor, *,
                           batch: int, n_heads: int, nq: int, n_tiles: int, dh: int, scale: float, totals_k_fp16: int = 0,
                           tag: Optional[str] = None, k_fp16: bool = False, stats: Optional[torch.Tensor] = None) -> BF:
    """attention_tiled_signed with the lists of bev_shared_lists: table rows that most scenes of the batch subtract are subtracted once.
    q BF [nq, d] (one copy for all batches); `totals_k_fp16` = the k_fp16 `totals` was computed with -> BF [batch*nq, d]."""
    qh, ql = q
    dev = qh.device
    d = n_heads * dh
    oh, ol = _bf_empty((batch * nq, d), dev, ql is not None)
    L = F.lib()
    nbytes = int(L.lvq_attention_tiled_signed_workspace_bytes(batch, n_heads, nq, n_tiles, dh))
    if nbytes == 0:
        raise F.LvqError(f"attention_tiled_shared: shape (nq={nq}, tiles={n_tiles}, dh={dh}) is not a long-stream shape")
    ws = F.workspace(nbytes, dev, "attn")
    with region(tag, dev):
        rc = L.lvq_attention_bf16_tiled_shared(F.ptr(qh), F.ptr(ql), F.ptr(kv), F.ptr(kv[:, d:]), F.ptr(row_src), F.ptr(list_src), F.ptr(list_info),
                                               list_src.shape[1], F.ptr(totals), int(totals_k_fp16), batch, n_heads, nq, n_tiles, dh,
                                               d, dh, 2 * d, dh, nq * d, d, dh, scale, 1 if k_fp16 else 0, F.ptr(oh), F.ptr(ol), F.ptr(stats),
                                               F.ptr(ws), ws.numel(), F.stream_ptr(dev))
    F.check(rc, f"lvq_attention_bf16_tiled_shared (B={batch}, H={n_heads}, nq={nq}, tiles={n_tiles})")
    return oh, ol


def stream_guard(q_hi: torch.Tensor, k_rows: torch.Tensor, n_heads: int, scale: float) -> torch.Tensor:
    """Per-model half of the plain-stream guard (include/lvq.h: lvq_stream_guard): q_hi [nq, >= n_heads * 64] bf16, k_rows [nkv, >= n_heads * 64]
    bf16 (row strides = q_hi.stride(0), k_rows.stride(0): column slices of a wider projection are taken as they are) -> g [n_heads, nq] fp32,
    g = (1 + max |score|) / sqrt(N_eff) per (head, query)."""
    F.require_cuda(q_hi[:1], k_rows[:1])                              # device only: rows may be strided, elements within a row may not
    assert q_hi.dtype == torch.bfloat16 and k_rows.dtype == torch.bfloat16 and q_hi.stride(1) == 1 and k_rows.stride(1) == 1
    nq, nkv = q_hi.shape[0], k_rows.shape[0]
    dev = q_hi.device
    L = F.lib()
    nbytes = int(L.lvq_stream_guard_workspace_bytes(nq, nkv))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)          # once per weights version: not cached
    g = torch.empty((n_heads, nq), dtype=torch.float32, device=dev)
    rc = L.lvq_stream_guard(F.ptr(q_hi), F.ptr(k_rows), n_heads, nq, nkv, q_hi.stride(0), k_rows.stride(0),
                            scale, F.ptr(g), F.ptr(ws), nbytes, F.stream_ptr(dev))
    F.check(rc, "lvq_stream_guard")
    return g


def scale_add_rows(x: torch.Tensor, add: Optional[torch.Tensor], alpha: float = 1.0) -> torch.Tensor:
    F.require_cuda(x, add)
    rows, d = x.shape
    out = torch.empty_like(x)
    rc = F.lib().lvq_scale_add_rows(F.ptr(x), F.ptr(add), add.shape[0] if add is not None else 0, alpha,
                                    rows, d, F.ptr(out), F.stream_ptr(x.device))
    F.check(rc, "lvq_scale_add_rows")
    return out


def rope_inplace(x: BF, rows: int, seq_len: int, n_heads: int, dh: int, ld: int, theta: float, pos0: int = 0):
    """Rotary embedding applied in place to a (column slice of a) packed projection; position = pos0 + row % seq_len."""
    hi, lo = x
    if pos0:
        rc = F.lib().lvq_rope_inplace_at(F.ptr(hi), F.ptr(lo), rows, seq_len, pos0, n_heads, dh,
                                         ld, theta, F.stream_ptr(hi.device))
        F.check(rc, "lvq_rope_inplace_at")
        return
    rc = F.lib().lvq_rope_inplace(F.ptr(hi), F.ptr(lo), rows, seq_len, n_heads, dh, ld,
                                  theta, F.stream_ptr(hi.device))
    F.check(rc, "lvq_rope_inplace")


def argmax_rows(x: torch.Tensor) -> torch.Tensor:
    """[rows, n] fp32 -> [rows] int64, first maximum of every row (greedy decoding)."""
    F.require_cuda(x)
    rows, n = x.shape
    out = torch.empty((rows,), dtype=torch.int64, device=x.device)
    F.check(F.lib().lvq_argmax_rows(F.ptr(x), rows, n, F.ptr(out), F.stream_ptr(x.device)), "lvq_argmax_rows")
    return out


def sample_rows(logits: torch.Tensor, temperature: float, top_k: int, top_p: float, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """[rows, vocab] fp32 -> [rows] int64 drawn like transformers' do_sample step (temperature -> top-k -> top-p -> multinomial,
    lvq_sample_rows).  The uniforms come from torch's RNG on the logits' device (seedable through `generator` / torch.manual_seed)."""
    F.require_cuda(logits)
    rows, n = logits.shape
    u = torch.rand((rows,), dtype=torch.float32, device=logits.device, generator=generator)
    out = torch.empty((rows,), dtype=torch.int64, device=logits.device)
    rc = F.lib().lvq_sample_rows(F.ptr(logits), rows, n, temperature, int(top_k or 0), top_p,
                                 F.ptr(u), F.ptr(out), F.stream_ptr(logits.device))
    F.check(rc, f"lvq_sample_rows (vocab={n}, top_k={top_k}: the top-k filter may only be disabled for vocab <= 1024)")
    return out


def swiglu(gate_up: torch.Tensor, split: bool) -> BF:
    rows, two_i = gate_up.shape
    hi, lo = _bf_empty((rows, two_i // 2), gate_up.device, split)
    rc = F.lib().lvq_swiglu(F.ptr(gate_up), rows, two_i // 2, F.ptr(hi), F.ptr(lo), F.stream_ptr(gate_up.device))
    F.check(rc, "lvq_swiglu")
    return hi, lo


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Mean CE over labels >= 0 (ignore_index -100): returns a 0-dim device tensor, no host sync."""
    rows, vocab = logits.shape
    acc = torch.zeros(2, dtype=torch.float32, device=logits.device)
    rc = F.lib().lvq_cross_entropy(F.ptr(logits), F.ptr(labels), rows, vocab, F.ptr(acc), F.stream_ptr(logits.device))
    F.check(rc, "lvq_cross_entropy")
    return acc[0] / acc[1]


GEMM_LN_WIDTHS = (256, 512, 768, 896, 1024)


def linear_ln_supported(n: int, k: int) -> bool:
    return n in GEMM_LN_WIDTHS and k % 32 == 0 and k <= 256


def linear_ln(a: BF, w: BF, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: Optional[torch.Tensor], eps: float,
              post: Optional[torch.Tensor] = None, tag: Optional[str] = None, out_lo: Optional[bool] = None) -> BF:
    """LayerNorm(a @ w.T + bias) * gamma + beta + post[row % rows] -> BF, no fp32 [M,N] intermediate (lvq_gemm_ln_bf16).
    out_lo=False: split operands, plain result (the "mixed" mode's BEV tokens)."""
    ah, al = a
    wh, wl = w
    m, k = ah.shape
    n = wh.shape[0]
    split = al is not None
    yh, yl = _bf_empty((m, n), ah.device, split if out_lo is None else (out_lo and split))
    with region(tag, ah.device):
        rc = F.lib().lvq_gemm_ln_bf16(F.ptr(ah), F.ptr(al), F.ptr(wh), F.ptr(wl), F.ptr(bias), F.ptr(gamma), F.ptr(beta), eps,
                                      F.ptr(post), post.shape[0] if post is not None else 0, m, n, k,
                                      k, k, F.ptr(yh), F.ptr(yl), F.stream_ptr(ah.device))
    F.check(rc, f"lvq_gemm_ln_bf16 (m={m}, n={n}, k={k})")
    return yh, yl


def _ws_query(fn, what: str, *args) -> int:
    """A `*_workspace_bytes(..., size_t *bytes)` query that returns a status."""
    n = ctypes.c_size_t(0)
    F.check(fn(*args, ctypes.byref(n)), what)
    return n.value


def _ws_or_none(query, dev, tag: str):
    """(pointer, bytes) of the workspace query(bytes_out) asks for; a refused query gives none, so that the call itself names the reason."""
    n = ctypes.c_size_t(0)
    if query(ctypes.byref(n)) != F.LVQ_OK:
        return F.ptr(None), 0
    ws = F.workspace(n.value, dev, tag)
    return F.ptr(ws), ws.numel()


def _decode_tables(what: str, dev, b: int, task_channels, task_n_cls, class_map, k: int, box_dim: int, stride: int, voxel_xy, range_xy,
                   limit_range, score_thresh: Optional[float], positive: bool = False):
    """center_decode's and voxel_decode's host tables checked -> (the four outputs, the ABI's arguments from n_tasks to counts)."""
    n_tasks = len(task_n_cls)
    if len(task_channels) != n_tasks or any(len(r) != 6 for r in task_channels) or len(class_map) != sum(int(c) for c in task_n_cls):
        raise F.LvqError(f"{what}: task_channels is [n_tasks][6], class_map holds sum(task_n_cls) entries")
    if positive and (b <= 0 or k <= 0):
        raise F.LvqError(f"{what}: batch = {b}, k = {k}")
    boxes = torch.empty((b, n_tasks, k, box_dim), dtype=torch.float32, device=dev)
    scores = torch.empty((b, n_tasks, k), dtype=torch.float32, device=dev)
    labels = torch.empty((b, n_tasks, k), dtype=torch.int32, device=dev)
    counts = torch.empty((b, n_tasks), dtype=torch.int32, device=dev)
    args = (n_tasks, F.i32x([c for row in task_channels for c in row]), F.i32x(task_n_cls), F.i32x(class_map), k, box_dim, stride,
            F.f32x(voxel_xy), F.f32x(range_xy), F.f32x(limit_range), -1.0 if score_thresh is None else float(score_thresh), F.ptr(boxes),
            F.ptr(scores), F.ptr(labels), F.ptr(counts))
    return (boxes, scores, labels, counts), args


def center_decode(maps: torch.Tensor, task_channels, task_n_cls, class_map, *, k: int, box_dim: int, stride: int, voxel_xy, range_xy,
                  limit_range, score_thresh: Optional[float], tag: Optional[str] = None):
    """lvq_center_decode.  maps [B, c_total, H, W] fp32; task_channels: per task the first channel of (center, center_z, dim, rot, vel or
    -1, hm); task_n_cls and class_map (the tasks' class-id mappings, concatenated) are host lists.  score_thresh None keeps every score.
    Returns (boxes [B, T, k, box_dim], scores [B, T, k], labels [B, T, k] int32, counts [B, T] int32): candidates in descending score
    order, equal scores towards the lower flat index, rows behind a count zero."""
    F.require_cuda(maps)
    if maps.dim() != 4 or maps.dtype != torch.float32:
        raise F.LvqError(f"center_decode: expected fp32 [B, C, H, W] maps, got {maps.dtype} {tuple(maps.shape)}")
    b, c_total, h, w = maps.shape
    dev, L = maps.device, F.lib()
    out, args = _decode_tables("center_decode", dev, b, task_channels, task_n_cls, class_map, k, box_dim, stride, voxel_xy, range_xy,
                               limit_range, score_thresh)
    n_tasks = len(task_n_cls)
    ws = _ws_or_none(lambda n: L.lvq_center_decode_workspace_bytes(b, n_tasks, max(int(c) for c in task_n_cls), h, w, n), dev, "center_head")
    with region(tag, dev):
        rc = L.lvq_center_decode(F.ptr(maps), b, c_total, h, w, *args, *ws, F.stream_ptr(dev))
    F.check(rc, f"lvq_center_decode (B={b}, {n_tasks} tasks, {h} x {w}, K={k})")
    return out


def boxes_iou_bev(boxes_a: torch.Tensor, boxes_b: torch.Tensor) -> torch.Tensor:
    """lvq_boxes_iou_bev: [N, 7] x [M, 7] fp32 (x, y, z, dx, dy, dz, heading) -> rotated BEV IoU [N, M]."""
    F.require_cuda(boxes_a, boxes_b)
    if boxes_a.dim() != 2 or boxes_b.dim() != 2 or boxes_a.shape[1] != 7 or boxes_b.shape[1] != 7 or boxes_a.dtype != torch.float32 or \
            boxes_b.dtype != torch.float32:
        raise F.LvqError(f"boxes_iou_bev: expected fp32 [N, 7] and [M, 7], got {tuple(boxes_a.shape)} and {tuple(boxes_b.shape)}")
    n, m = boxes_a.shape[0], boxes_b.shape[0]
    out = torch.empty((n, m), dtype=torch.float32, device=boxes_a.device)
    if n and m:
        F.check(F.lib().lvq_boxes_iou_bev(F.ptr(boxes_a), n, F.ptr(boxes_b), m, F.ptr(out), F.stream_ptr(out.device)), "lvq_boxes_iou_bev")
    return out


def _nms(fn, ws_fn, what: str, ws_tag: str, boxes: torch.Tensor, counts: torch.Tensor, thresh: float, pre_max: int, post_max: int, tag):
    """The entry point `fn` (lvq_nms_bev / lvq_nms_bev_wide) and its workspace query `ws_fn` behind nms_bev / nms_bev_wide (`what`)."""
    F.require_cuda(boxes, counts)
    if boxes.dim() != 3 or boxes.dtype != torch.float32 or counts.dtype != torch.int32 or counts.numel() != boxes.shape[0]:
        raise F.LvqError(f"{what}: expected fp32 boxes [G, N, >= 7] and int32 counts [G], got {tuple(boxes.shape)} and {tuple(counts.shape)}")
    g, n_max, stride = boxes.shape
    dev = boxes.device
    keep = torch.empty((g, post_max), dtype=torch.int32, device=dev)
    keep_count = torch.empty((g,), dtype=torch.int32, device=dev)
    ws = F.workspace(_ws_query(ws_fn, f"{ws_fn.__name__} ({g} groups of {n_max})", g, n_max), dev, ws_tag)
    with region(tag, dev):
        rc = fn(F.ptr(boxes), stride, F.ptr(counts), g, n_max, int(pre_max), int(post_max), float(thresh), F.ptr(keep), F.ptr(keep_count),
                F.ptr(ws), ws.numel(), F.stream_ptr(dev))
    F.check(rc, f"{fn.__name__} ({g} groups of {n_max})")
    return keep, keep_count


def nms_bev(boxes: torch.Tensor, counts: torch.Tensor, *, thresh: float, pre_max: int, post_max: int, tag: Optional[str] = None):
    """lvq_nms_bev.  boxes [G, N_max, >= 7] fp32, each group in descending score order; counts [G] int32 on the device.
    Returns (keep [G, post_max] int32: kept row numbers ascending, -1 behind the count; keep_count [G] int32).  No host read."""
    L = F.lib()
    return _nms(L.lvq_nms_bev, L.lvq_nms_bev_workspace_bytes, "nms_bev", "center_head_nms", boxes, counts, thresh, pre_max, post_max, tag)


def center_collect(boxes: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor, keep: torch.Tensor, keep_count: torch.Tensor,
                   tag: Optional[str] = None):
    """lvq_center_collect: the kept rows of every scene's tasks in head order -> (boxes [B, T * post_max, D], scores, labels int64
    1-based, count [B] int32); rows behind a scene's count are not written."""
    F.require_cuda(boxes, scores, labels, keep, keep_count)
    b, t, k, d = boxes.shape
    post_max, dev = keep.shape[-1], boxes.device
    out_b = torch.empty((b, t * post_max, d), dtype=torch.float32, device=dev)
    out_s = torch.empty((b, t * post_max), dtype=torch.float32, device=dev)
    out_l = torch.empty((b, t * post_max), dtype=torch.int64, device=dev)
    out_n = torch.empty((b,), dtype=torch.int32, device=dev)
    with region(tag, dev):
        rc = F.lib().lvq_center_collect(F.ptr(boxes), F.ptr(scores), F.ptr(labels), F.ptr(keep), F.ptr(keep_count), b, t, k, d, post_max,
                                        F.ptr(out_b), F.ptr(out_s), F.ptr(out_l), F.ptr(out_n), F.stream_ptr(dev))
    F.check(rc, "lvq_center_collect")
    return out_b, out_s, out_l, out_n


HEAD_TASK_C = 16               # output channels per task in the head buffer of sparse_head / voxel_decode


def sparse_head(feat: torch.Tensor, nbr: Optional[torch.Tensor], *, k_vol: int, task_n_br, chan_owner, num_conv: int, br_stride: int,
                w_hi: Optional[torch.Tensor], w_lo: Optional[torch.Tensor], scale: Optional[torch.Tensor], shift: Optional[torch.Tensor],
                w_last: torch.Tensor, bias: torch.Tensor, tag: Optional[str] = None) -> torch.Tensor:
    """lvq_sparse_head.  feat [N, 128] fp32; nbr [N, k_vol] int32 or None (k_vol 1: row i reads row i); task_n_br and chan_owner
    ([n_tasks][<= 16] owning branch, negative = nobody) are host lists; w_hi / w_lo [n_tasks, br_stride, k_vol, 128, 128] packed bf16
    (w_lo None: plain bf16), scale / shift [n_tasks, br_stride, 128], w_last [n_tasks, 16, 128], bias [n_tasks, 16] fp32.
    Returns the head buffer, CHANNEL-major [16 * n_tasks, N] fp32; channels nobody owns are zeros."""
    F.require_cuda(feat, nbr, w_hi, w_lo, scale, shift, w_last, bias)
    if feat.dim() != 2 or feat.dtype != torch.float32:
        raise F.LvqError(f"sparse_head: expected fp32 [N, C] features, got {feat.dtype} {tuple(feat.shape)}")
    n, c_in = feat.shape
    n_tasks, dev = len(task_n_br), feat.device
    task_c = max(len(r) for r in chan_owner) if len(chan_owner) else 0
    if len(chan_owner) != n_tasks or any(len(r) != task_c for r in chan_owner):
        raise F.LvqError("sparse_head: chan_owner is [n_tasks][task_c]")
    if nbr is not None and (nbr.dtype != torch.int32 or tuple(nbr.shape) != (n, k_vol)):
        raise F.LvqError(f"sparse_head: nbr is int32 [N, k_vol], got {nbr.dtype} {tuple(nbr.shape)}")
    out = torch.empty((HEAD_TASK_C * n_tasks, n), dtype=torch.float32, device=dev)
    with region(tag, dev):
        rc = F.lib().lvq_sparse_head(F.ptr(feat), n, c_in, F.ptr(nbr), int(k_vol), n_tasks, F.i32x(task_n_br), int(br_stride),
                                     F.i32x([c for row in chan_owner for c in row]), task_c, int(num_conv), F.ptr(w_hi), F.ptr(w_lo),
                                     F.ptr(scale), F.ptr(shift), F.ptr(w_last), F.ptr(bias), F.ptr(out), F.stream_ptr(dev))
    F.check(rc, f"lvq_sparse_head (N={n}, C={c_in}, k_vol={k_vol}, {n_tasks} tasks, num_conv={num_conv})")
    return out


def voxel_decode(head: torch.Tensor, indices: torch.Tensor, batch: int, task_channels, task_n_cls, class_map, *, k: int, box_dim: int,
                 stride: int, voxel_xy, range_xy, limit_range, score_thresh: Optional[float], tag: Optional[str] = None):
    """lvq_voxel_decode.  head [c_total, N] fp32 (sparse_head's buffer), indices [N, 3] int32 (b, y, x); the host tables and the geometry
    are center_decode's.  Returns (boxes [B, T, k, box_dim], scores [B, T, k], labels [B, T, k] int32, counts [B, T] int32): per (scene,
    task) the min(k, n_cls * n_b) best rows of the scene in descending score order, equal scores towards the lower (class, stored row),
    rows behind a count zero."""
    F.require_cuda(head, indices)
    if head.dim() != 2 or head.dtype != torch.float32 or indices.dtype != torch.int32 or tuple(indices.shape) != (head.shape[1], 3):
        raise F.LvqError(f"voxel_decode: expected fp32 [C, N] head and int32 [N, 3] indices, got {head.dtype} {tuple(head.shape)} and "
                         f"{indices.dtype} {tuple(indices.shape)}")
    c_total, n = head.shape
    n_tasks, dev, b, L = len(task_n_cls), head.device, int(batch), F.lib()
    out, args = _decode_tables("voxel_decode", dev, b, task_channels, task_n_cls, class_map, k, box_dim, stride, voxel_xy, range_xy,
                               limit_range, score_thresh, positive=True)
    ws = _ws_or_none(lambda nb: L.lvq_voxel_decode_workspace_bytes(b, n_tasks, max(int(c) for c in task_n_cls), n, nb), dev, "center_head")
    with region(tag, dev):
        rc = L.lvq_voxel_decode(F.ptr(head), F.ptr(indices), n, b, c_total, *args, *ws, F.stream_ptr(dev))
    F.check(rc, f"lvq_voxel_decode (B={b}, {n_tasks} tasks, {n} rows, K={k})")
    return out


def anchor_decode(maps: torch.Tensor, anchors: torch.Tensor, *, n_anchors: int, n_cls: int, cls_channel: int, box_channel: int,
                  dir_channel: int = -1, n_dir_bins: int = 0, dir_offset: float = 0.0, dir_limit_offset: float = 0.0,
                  score_thresh: Optional[float] = None, tag: Optional[str] = None):
    """lvq_anchor_decode.  maps [B, c_total, H, W] fp32 (cls | box | dir channels from the given first channels; dir_channel -1: no
    direction classifier), anchors [H * W * n_anchors, 7] fp32 in the flat order (y, x, a).  Returns (cls_preds [B, N, n_cls], box_preds
    [B, N, 7], scores [B, N], labels [B, N] int32 0-based, cand, cand_count): with a score_thresh, cand [B, N] int32 holds in its first
    cand_count[b] entries the anchors with score >= score_thresh, in no particular order; without one both are None."""
    F.require_cuda(maps, anchors)
    if maps.dim() != 4 or maps.dtype != torch.float32 or not maps.is_contiguous():
        raise F.LvqError(f"anchor_decode: expected contiguous fp32 [B, C, H, W] maps, got {maps.dtype} {tuple(maps.shape)}")
    b, c_total, h, w = maps.shape
    n, dev = h * w * int(n_anchors), maps.device
    if anchors.dtype != torch.float32 or tuple(anchors.shape) != (n, 7) or not anchors.is_contiguous():
        raise F.LvqError(f"anchor_decode: expected contiguous fp32 anchors [{n}, 7], got {anchors.dtype} {tuple(anchors.shape)}")
    cls_preds = torch.empty((b, n, n_cls), dtype=torch.float32, device=dev)
    box_preds = torch.empty((b, n, 7), dtype=torch.float32, device=dev)
    scores = torch.empty((b, n), dtype=torch.float32, device=dev)
    labels = torch.empty((b, n), dtype=torch.int32, device=dev)
    cand = cand_count = None
    if score_thresh is not None:
        cand = torch.empty((b, n), dtype=torch.int32, device=dev)
        cand_count = torch.empty((b,), dtype=torch.int32, device=dev)
    with region(tag, dev):
        rc = F.lib().lvq_anchor_decode(F.ptr(maps), b, c_total, h, w, int(cls_channel), int(box_channel), int(dir_channel), int(n_anchors),
                                       int(n_cls), int(n_dir_bins), float(dir_offset), float(dir_limit_offset), F.ptr(anchors),
                                       0.0 if score_thresh is None else float(score_thresh), F.ptr(cls_preds), F.ptr(box_preds),
                                       F.ptr(scores), F.ptr(labels), F.ptr(cand), F.ptr(cand_count), F.stream_ptr(dev))
    F.check(rc, f"lvq_anchor_decode (B={b}, {h} x {w}, {n_anchors} anchors, {n_cls} classes)")
    return cls_preds, box_preds, scores, labels, cand, cand_count


def anchor_select(scores: torch.Tensor, labels: torch.Tensor, box_preds: torch.Tensor, *, score_thresh: Optional[float], pre_max: int,
                  cand: Optional[torch.Tensor] = None, cand_count: Optional[torch.Tensor] = None, tag: Optional[str] = None):
    """lvq_anchor_select.  scores [B, N] fp32, labels [B, N] int32, box_preds [B, N, 7] fp32; score_thresh None takes every anchor.
    Returns (sel_boxes [B, pre_max, 7], sel_scores, sel_labels int32, sel_index int32, sel_count [B] int32): per scene the
    min(pre_max, candidates) best in descending score order, equal scores towards the lower anchor index; rows behind a count are zeros
    with index -1.  cand / cand_count: anchor_decode's candidate set for the same threshold (the scan is skipped)."""
    F.require_cuda(scores, labels, box_preds, cand, cand_count)
    if scores.dim() != 2 or scores.dtype != torch.float32 or labels.dtype != torch.int32 or labels.shape != scores.shape or \
            box_preds.dtype != torch.float32 or tuple(box_preds.shape) != (*scores.shape, 7) or \
            not (scores.is_contiguous() and labels.is_contiguous() and box_preds.is_contiguous()):
        raise F.LvqError(f"anchor_select: expected contiguous fp32 scores [B, N], int32 labels [B, N] and fp32 boxes [B, N, 7], got "
                         f"{tuple(scores.shape)}, {tuple(labels.shape)} and {tuple(box_preds.shape)}")
    b, n = scores.shape
    if (cand is None) != (cand_count is None) or (cand is not None and (cand.dtype != torch.int32 or tuple(cand.shape) != (b, n) or
                                                                         cand_count.dtype != torch.int32 or cand_count.numel() != b)):
        raise F.LvqError("anchor_select: cand is int32 [B, N] and cand_count int32 [B], or both are None")
    dev, L, pre_max = scores.device, F.lib(), int(pre_max)
    rows = max(pre_max, 1)
    sel_boxes = torch.empty((b, rows, 7), dtype=torch.float32, device=dev)
    sel_scores = torch.empty((b, rows), dtype=torch.float32, device=dev)
    sel_labels = torch.empty((b, rows), dtype=torch.int32, device=dev)
    sel_index = torch.empty((b, rows), dtype=torch.int32, device=dev)
    sel_count = torch.empty((b,), dtype=torch.int32, device=dev)
    ws = _ws_or_none(lambda nb: L.lvq_anchor_select_workspace_bytes(b, n, nb), dev, "anchor_head")
    with region(tag, dev):
        rc = L.lvq_anchor_select(F.ptr(scores), F.ptr(labels), F.ptr(box_preds), b, n, int(score_thresh is not None),
                                 0.0 if score_thresh is None else float(score_thresh), pre_max, F.ptr(cand), F.ptr(cand_count),
                                 F.ptr(sel_boxes), F.ptr(sel_scores), F.ptr(sel_labels), F.ptr(sel_index), F.ptr(sel_count), *ws,
                                 F.stream_ptr(dev))
    F.check(rc, f"lvq_anchor_select (B={b}, N={n}, pre_max={pre_max})")
    return sel_boxes, sel_scores, sel_labels, sel_index, sel_count


def nms_bev_wide(boxes: torch.Tensor, counts: torch.Tensor, *, thresh: float, pre_max: int, post_max: int, tag: Optional[str] = None):
    """lvq_nms_bev_wide: nms_bev for groups of up to 4096 rows.  boxes [G, N_max, >= 7] fp32, each group in descending score order;
    counts [G] int32 on the device.  Returns (keep [G, post_max] int32, keep_count [G] int32).  No host read."""
    L = F.lib()
    return _nms(L.lvq_nms_bev_wide, L.lvq_nms_bev_wide_workspace_bytes, "nms_bev_wide", "anchor_head_nms", boxes, counts, thresh, pre_max, post_max,
                tag)


def heatmap_proposals(maps: torch.Tensor, *, first_channel: int, n_cls: int, point_class_mask: int, n_proposals: int, nms_kernel_size: int = 3,
                      tag: Optional[str] = None):
    """lvq_heatmap_proposals.  maps [B, c_total, H, W] fp32 with the heat-map logits in channels first_channel .. + n_cls - 1;
    point_class_mask: bit c set = class c keeps every cell (no 3 x 3 suppression).  Returns (prop_flat [B, P] int32, prop_score [B, P],
    query_heatmap_score [B, n_cls, P]): the P largest surviving heats in descending order, equal values towards the lower flat index."""
    F.require_cuda(maps)
    if maps.dim() != 4 or maps.dtype != torch.float32:
        raise F.LvqError(f"heatmap_proposals: expected fp32 [B, C, H, W] maps, got {maps.dtype} {tuple(maps.shape)}")
    b, c_total, h, w = maps.shape
    dev, L, p = maps.device, F.lib(), int(n_proposals)
    rows = max(p, 1)
    flat = torch.empty((b, rows), dtype=torch.int32, device=dev)
    score = torch.empty((b, rows), dtype=torch.float32, device=dev)
    qhs = torch.empty((b, max(int(n_cls), 1), rows), dtype=torch.float32, device=dev)
    ws = _ws_or_none(lambda nb: L.lvq_heatmap_proposals_workspace_bytes(b, int(n_cls), h, w, nb), dev, "transfusion_head")
    with region(tag, dev):
        rc = L.lvq_heatmap_proposals(F.ptr(maps), b, c_total, h, w, int(first_channel), int(n_cls), int(point_class_mask), int(nms_kernel_size),
                                     p, F.ptr(flat), F.ptr(score), F.ptr(qhs), *ws, F.stream_ptr(dev))
    F.check(rc, f"lvq_heatmap_proposals (B={b}, {n_cls} classes, {h} x {w}, P={p}, NMS_KERNEL_SIZE={nms_kernel_size})")
    return flat, score, qhs


def pos_embed_learned(pos: torch.Tensor, w1: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
                      tag: Optional[str] = None) -> torch.Tensor:
    """lvq_pos_embed_learned.  pos [n, 2] fp32; w1 [d, 2], scale / shift [d] (BatchNorm1d and the first conv's bias folded), w2 [d_out, d],
    b2 [d_out] -> [n, d_out] fp32."""
    F.require_cuda(pos, w1, scale, shift, w2, b2)
    if pos.dim() != 2 or pos.shape[1] != 2 or pos.dtype != torch.float32:
        raise F.LvqError(f"pos_embed_learned: expected fp32 [n, 2] positions, got {pos.dtype} {tuple(pos.shape)}")
    n, d, d_out = pos.shape[0], w1.shape[0], w2.shape[0]
    if tuple(w1.shape) != (d, 2) or tuple(w2.shape) != (d_out, d) or any(tuple(t.shape) != (d,) for t in (scale, shift)) or \
            tuple(b2.shape) != (d_out,):
        raise F.LvqError(f"pos_embed_learned: w1 {tuple(w1.shape)}, w2 {tuple(w2.shape)} and the vectors do not agree on d, d_out")
    out = torch.empty((n, d_out), dtype=torch.float32, device=pos.device)
    with region(tag, pos.device):
        rc = F.lib().lvq_pos_embed_learned(F.ptr(pos), n, d, d_out, F.ptr(w1), F.ptr(scale), F.ptr(shift), F.ptr(w2), F.ptr(b2), F.ptr(out),
                                           F.stream_ptr(pos.device))
    F.check(rc, f"lvq_pos_embed_learned (n={n}, d={d})")
    return out


def transfusion_queries(feat_hi: torch.Tensor, feat_lo: Optional[torch.Tensor], prop_flat: torch.Tensor, *, n_cls: int, y_size: int,
                        class_w: torch.Tensor, class_b: torch.Tensor, pe, tag: Optional[str] = None):
    """lvq_transfusion_queries.  feat_hi (+ feat_lo) [B, H, W, d] 16-bit planes, prop_flat [B, P] int32, class_w [d, n_cls], class_b [d],
    pe = (w1, scale, shift, w2, b2) of pos_embed_learned.  Returns (query_feat [B, P, d], query_pos [B, P, 2], query_labels [B, P] int32,
    query_pe [B, P, d])."""
    F.require_cuda(feat_hi, feat_lo, prop_flat, class_w, class_b, *pe)
    if feat_hi.dim() != 4 or feat_hi.element_size() != 2 or prop_flat.dtype != torch.int32 or prop_flat.dim() != 2 or \
            prop_flat.shape[0] != feat_hi.shape[0]:
        raise F.LvqError(f"transfusion_queries: expected 16-bit planes [B, H, W, d] and int32 prop_flat [B, P], got {tuple(feat_hi.shape)} and "
                         f"{prop_flat.dtype} {tuple(prop_flat.shape)}")
    b, h, w, d = feat_hi.shape
    p, dev = prop_flat.shape[1], feat_hi.device
    if tuple(class_w.shape) != (d, int(n_cls)) or tuple(class_b.shape) != (d,) or tuple(pe[3].shape) != (d, d):
        raise F.LvqError(f"transfusion_queries: class_w {tuple(class_w.shape)}, class_b {tuple(class_b.shape)}, pe w2 {tuple(pe[3].shape)} with d = {d}")
    feat = torch.empty((b, p, d), dtype=torch.float32, device=dev)
    pos = torch.empty((b, p, 2), dtype=torch.float32, device=dev)
    labels = torch.empty((b, p), dtype=torch.int32, device=dev)
    qpe = torch.empty((b, p, d), dtype=torch.float32, device=dev)
    with region(tag, dev):
        rc = F.lib().lvq_transfusion_queries(F.ptr(feat_hi), F.ptr(feat_lo), b, h, w, d, F.ptr(prop_flat), p, int(n_cls), int(y_size),
                                             F.ptr(class_w), F.ptr(class_b), *[F.ptr(t) for t in pe], F.ptr(feat), F.ptr(pos), F.ptr(labels),
                                             F.ptr(qpe), F.stream_ptr(dev))
    F.check(rc, f"lvq_transfusion_queries (B={b}, {h} x {w}, d={d}, P={p})")
    return feat, pos, labels, qpe


def transfusion_add_pe(x: torch.Tensor, pe: torch.Tensor, split: bool) -> BF:
    """lvq_transfusion_add_pe: x + pe (fp32, same shape) as a bf16 operand (hi, lo with `split`)."""
    F.require_cuda(x, pe)
    if x.shape != pe.shape or x.dtype != torch.float32 or pe.dtype != torch.float32:
        raise F.LvqError(f"transfusion_add_pe: expected two fp32 tensors of one shape, got {tuple(x.shape)} and {tuple(pe.shape)}")
    hi, lo = _bf_empty(x.shape, x.device, split)
    F.check(F.lib().lvq_transfusion_add_pe(F.ptr(x), F.ptr(pe), x.numel(), F.ptr(hi), F.ptr(lo), F.stream_ptr(x.device)),
            "lvq_transfusion_add_pe")
    return hi, lo


def transfusion_tail(x: torch.Tensor, query_pos: torch.Tensor, query_labels: torch.Tensor, prop_score: torch.Tensor, *, n_cls: int,
                     has_vel: bool, ffn, norm, heads, eps: float, stride: int, voxel_xy, range_xy, limit_range, score_thresh: float,
                     tag: Optional[str] = None):
    """lvq_transfusion_tail.  x [B, P, 128] fp32 (after norm2); ffn = (w1 [F, 128], b1, w2 [128, F], b2), norm = (gamma, beta),
    heads = (w1 [nb * 64, 128], scale, shift, w2 [c_total, 64], b2).  Returns (raw [B, c_total, P], boxes [B, P, 9 | 7], scores [B, P],
    labels [B, P] int32 1-based, counts [B] int32): the kept rows in proposal order, zeros behind a count."""
    F.require_cuda(x, query_pos, query_labels, prop_score, *ffn, *norm, *heads)
    if x.dim() != 3 or x.dtype != torch.float32 or x.shape[2] != 128:
        raise F.LvqError(f"transfusion_tail: expected fp32 [B, P, 128] rows, got {x.dtype} {tuple(x.shape)}")
    b, p, _ = x.shape
    f, dev, L = ffn[0].shape[0], x.device, F.lib()
    c_box = 10 if has_vel else 8
    nb, c_total, box_dim = (6 if has_vel else 5), c_box + int(n_cls), (9 if has_vel else 7)
    want = [(tuple(query_pos.shape), (b, p, 2)), (tuple(query_labels.shape), (b, p)), (tuple(prop_score.shape), (b, p)),
            (tuple(ffn[0].shape), (f, 128)), (tuple(ffn[1].shape), (f,)), (tuple(ffn[2].shape), (128, f)), (tuple(ffn[3].shape), (128,)),
            (tuple(norm[0].shape), (128,)), (tuple(norm[1].shape), (128,)), (tuple(heads[0].shape), (nb * 64, 128)),
            (tuple(heads[1].shape), (nb * 64,)), (tuple(heads[2].shape), (nb * 64,)), (tuple(heads[3].shape), (c_total, 64)),
            (tuple(heads[4].shape), (c_total,))]
    if any(g != w_ for g, w_ in want) or query_labels.dtype != torch.int32:
        raise F.LvqError(f"transfusion_tail: operand shapes (got, expected) {[gw for gw in want if gw[0] != gw[1]]}, int32 labels")
    raw = torch.empty((b, c_total, p), dtype=torch.float32, device=dev)
    boxes = torch.empty((b, p, box_dim), dtype=torch.float32, device=dev)
    scores = torch.empty((b, p), dtype=torch.float32, device=dev)
    labels = torch.empty((b, p), dtype=torch.int32, device=dev)
    counts = torch.empty((b,), dtype=torch.int32, device=dev)
    ws = _ws_or_none(lambda nb: L.lvq_transfusion_tail_workspace_bytes(b, p, box_dim, nb), dev, "transfusion_tail")
    with region(tag, dev):
        rc = L.lvq_transfusion_tail(F.ptr(x), F.ptr(query_pos), F.ptr(query_labels), F.ptr(prop_score), b, p, f, int(n_cls), int(has_vel),
                                    *[F.ptr(t) for t in ffn], *[F.ptr(t) for t in norm], float(eps), *[F.ptr(t) for t in heads], int(stride),
                                    F.f32x(voxel_xy), F.f32x(range_xy), F.f32x(limit_range), float(score_thresh), F.ptr(raw), F.ptr(boxes),
                                    F.ptr(scores), F.ptr(labels), F.ptr(counts), *ws, F.stream_ptr(dev))
    F.check(rc, f"lvq_transfusion_tail (B={b}, P={p}, FFN={f}, {n_cls} classes)")
    return raw, boxes, scores, labels, counts
