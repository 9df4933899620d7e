"""Fusion side of the hot path with the reference's nn.Module API, MI355X-native.

Drop-in for (citations relative to /root/reference/src/):
  VATBlock        encoder-decoder/training/models/vat_blocks.py:7-47
  VATLiDAR        encoder-decoder/training/models/vat_lidar.py:42-304
  VATVision       encoder-decoder/training/models/vat_vision.py:20-235
  VisionAdapter   encoder-decoder/training/models/vision_adapter.py:35-145
  sdp_attention   deepencoder/clip_sdpa.py:50-66 (== sam_vary_sdpa.py:27-42)
  deepencoder_fuse  deepencoder/deepencoder_infer.py:505-511 + build_linear.py:18-19

Same constructor signatures, same `state_dict()` keys and shapes (SURVEY.md Appendix D -- torch's
nn.LayerNorm / nn.Linear / nn.MultiheadAttention / nn.Conv2d objects are kept as PARAMETER CONTAINERS so
checkpoints load unchanged and default initialisation consumes the RNG exactly like the reference),
same forward signatures, fp32 in / fp32 out.  The inference forward (eval() under torch.no_grad(), the reference's hot path) never
calls those containers: all arithmetic runs in liblvq_hip.so (bf16 MFMA, fp32 statistics/accumulation), and there is no fallback for it.

The kernels are forward-only.  A call in train() mode, or in grad mode with a trainable parameter or input, takes the autograd route
instead (autograd_route.py: the containers as ordinary torch modules; SURVEY 8b: "must fall back to torch ops when
torch.is_grad_enabled()"), so the reference's trainer can differentiate through the same objects; it warns once per class.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _ffi as F
from . import autograd_route as AG
from . import ops
from .ops import BF

NUM_VIEWS = 6  # vat_lidar.py:39
CAM_VIEWS = ("CAM_FRONT", "CAM_FRONT_RIGHT", "CAM_FRONT_LEFT", "CAM_BACK", "CAM_BACK_RIGHT", "CAM_BACK_LEFT")


class _HipModule(nn.Module):
    """Shared plumbing: precision switch, bf16 weight cache keyed on the parameter version."""

    def __init__(self):
        super().__init__()
        object.__setattr__(self, "_wcache", {})
        self.precision: Optional[str] = None   # None -> ops.default_precision()

    def _mode(self) -> str:
        return self.precision or ops.default_precision()

    def _split(self) -> bool:
        """Operands travel as hi + lo (bf16x3, and mixed outside its plain key stream)."""
        return self._mode() in ("bf16x3", "mixed", "mixed16")

    def _stream_plain(self, nq: int, nkv: int, dh: int) -> bool:
        """mixed mode, and the K/V side of this attention is a long key stream whose per-key roundings average out: x, K, V, P
        stay plain bf16 there (ops docstring) while the weights and the query side keep their lo parts."""
        return self._mode() in ("mixed", "mixed16") and ops.attention_stream_ok(nq, nkv, dh)

    def _w(self, p: torch.Tensor, pad_k: int = 0) -> BF:
        """bf16 (hi[, lo]) copy of a weight matrix [N,K]; rebuilt when the parameter changes."""
        split = self._split()

        def build():
            w = p.detach().reshape(p.shape[0], -1).float()
            if pad_k and w.shape[1] % pad_k:
                w = torch.nn.functional.pad(w, (0, pad_k - w.shape[1] % pad_k))
            return ops.cast(w.contiguous(), split)
        return F.derived(self._wcache, (id(p), split), (p,), build)

    def _guard(self, *tensors):
        """The HIP route: eval() under no_grad() on CUDA tensors, or a loud error (callers ask _autograd() first)."""
        if AG.wanted(self, *tensors):
            raise F.LvqError(f"{type(self).__name__}: this entry point has no autograd route; call it in eval() mode under torch.no_grad()")
        F.require_cuda(*[t for t in tensors if t is not None])

    def _autograd(self, *tensors) -> bool:
        """True when this call belongs to the autograd route (train() mode or gradients needed): torch ops, see autograd_route.py."""
        if AG.wanted(self, *tensors):
            AG.note(self)
            return True
        return False


def _f32(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    return (t if t.dtype == torch.float32 else t.float()).contiguous()


class VATBlock(_HipModule):
    """q [B,nq,d], kv [B,N_kv,d] -> [B,nq,d]: pre-LN self-attn, pre-LN cross-attn(q -> kv), pre-LN MLP."""

    def __init__(self, d_model: int, n_heads: int, d_mlp: int, dropout: float):
        super().__init__()
        self.sa_ln = nn.LayerNorm(d_model)
        self.sa = nn.MultiheadAttention(d_model, n_heads, dropout=dropout, batch_first=True)
        self.ca_ln = nn.LayerNorm(d_model)
        self.ca = nn.MultiheadAttention(d_model, n_heads, dropout=dropout, batch_first=True)
        self.mlp_ln = nn.LayerNorm(d_model)
        self.mlp = nn.Sequential(nn.Linear(d_model, d_mlp), nn.GELU(), nn.Dropout(dropout), nn.Linear(d_mlp, d_model),
                                 nn.Dropout(dropout))
        self.d_model, self.n_heads = d_model, n_heads
        self.fused_ca_in_block = False        # parity-true modes: fp16 fused cross-attention inside forward() too (see forward_tokens)
        if d_model % n_heads or (d_model // n_heads) % 8:
            raise ValueError("head_dim must be a multiple of 8 for the MFMA attention kernels")

    # ---- pieces (2-D token-major tensors) -------------------------------------------------------
    def _self_attn(self, q2: torch.Tensor, B: int, nq: int) -> torch.Tensor:
        d, h = self.d_model, self.n_heads
        dh = d // h
        split = self._split()
        _, qn = ops.layernorm(q2, self.sa_ln.weight, self.sa_ln.bias, self.sa_ln.eps, split)
        _, qkv = ops.linear(qn, self._w(self.sa.in_proj_weight), self.sa.in_proj_bias, out_bf=True)
        sl = lambda t, c: (t[0][:, c * d:], None if t[1] is None else t[1][:, c * d:])
        st = (nq * 3 * d, 3 * d, dh)
        o = ops.attention(sl(qkv, 0), sl(qkv, 1), sl(qkv, 2), batch=B, n_heads=h, n_kv_heads=h, nq=nq, nkv=nq, dh=dh,
                          q_strides=st, k_strides=st, v_strides=st, scale=1.0 / math.sqrt(dh))
        y, _ = ops.linear(o, self._w(self.sa.out_proj.weight), self.sa.out_proj.bias, residual=q2, out_f32=True)
        return y

    def project_kv(self, kv_bf: BF) -> BF:
        """K|V projection of the cross-attention: [B*Nkv, d] -> [B*Nkv, 2d] (rows d..3d of in_proj).  A plain kv_bf under split
        weights (mixed mode, long stream) gives plain K|V from a @ (w_hi + w_lo)."""
        d = self.d_model
        _, kvp = ops.linear(kv_bf, self._w(self.ca.in_proj_weight), self.ca.in_proj_bias, out_bf=True, w_rows=(d, 3 * d),
                            tag="ca_kv_proj")
        return kvp

    def _cross_attn(self, q2: torch.Tensor, kvp: BF, B: int, nq: int, nkv: int) -> torch.Tensor:
        d, h = self.d_model, self.n_heads
        dh = d // h
        split = self._split()
        _, qn = ops.layernorm(q2, self.ca_ln.weight, self.ca_ln.bias, self.ca_ln.eps, split)
        _, qp = ops.linear(qn, self._w(self.ca.in_proj_weight), self.ca.in_proj_bias, out_bf=True, w_rows=(0, d), tag="ca_q_proj")
        vsl = (kvp[0][:, d:], None if kvp[1] is None else kvp[1][:, d:])
        o = ops.attention(qp, kvp, vsl, batch=B, n_heads=h, n_kv_heads=h, nq=nq, nkv=nkv, dh=dh,
                          q_strides=(nq * d, d, dh), k_strides=(nkv * 2 * d, 2 * d, dh), v_strides=(nkv * 2 * d, 2 * d, dh),
                          scale=1.0 / math.sqrt(dh), tag="ca_attn")
        y, _ = ops.linear(o, self._w(self.ca.out_proj.weight), self.ca.out_proj.bias, residual=q2, out_f32=True, tag="ca_out_proj")
        return y

    # ---- first block of VATLiDAR: the query side does not depend on the scene (vat_lidar.py:259-270 -> vat_blocks.py:37-42) ----
    def shared_query_side(self, q1: torch.Tensor, nq: int) -> Tuple[torch.Tensor, BF]:
        """q1 [nq, d] fp32 (ONE copy of the learned queries) -> (q after self-attention [nq, d] fp32, Q projection of the
        cross-attention BF [nq, d]): computed once per step instead of once per scene."""
        d = self.d_model
        q2 = self._self_attn(q1, 1, nq)
        _, qn = ops.layernorm(q2, self.ca_ln.weight, self.ca_ln.bias, self.ca_ln.eps, self._split())
        _, qp = ops.linear(qn, self._w(self.ca.in_proj_weight), self.ca.in_proj_bias, out_bf=True, w_rows=(0, d), tag="ca_q_proj")
        return q2, qp

    def forward_tokens_tiled_signed(self, q2_1: torch.Tensor, qp: BF, totals: torch.Tensor, x_rows: BF, kv: torch.Tensor, row_src: torch.Tensor,
                                    rows_dev: torch.Tensor, B: int, nq: int, n_tiles: int, k_fp16: bool = False,
                                    stats: Optional[torch.Tensor] = None, totals_k_fp16: int = 0) -> torch.Tensor:
        """forward_tokens_tiled for scene-independent queries: the attention streams each scene's DIRTY rows only (twice: the computed
        rows added, the table rows of the same cells subtracted from the per-model `totals`), csrc/attention.hip `signed pair stream`.
        Batches of three or more scenes subtract the table rows that most of their scenes have dirty once per call (`shared subtraction`,
        include/lvq.h: lvq_bev_shared_lists); LVQ_NO_SHARED_SUBTRACT=1 keeps the per-scene pair lists.  `totals_k_fp16`: the k_fp16
        `totals` was computed with."""
        d, h = self.d_model, self.n_heads
        dh = d // h
        hw = n_tiles * 64
        if x_rows is not None:                                  # unfused route: tokens -> K|V GEMM; the fused kernel has filled kv[hw:] already
            ops.linear_live_rows(x_rows, self._w(self.ca.in_proj_weight), self.ca.in_proj_bias, rows_dev, (d, 3 * d), tag="ca_kv_proj", out=kv[hw:])
        # The shared lists make a scene's bits depend on the other scenes of its batch (fp32 accumulation order only).  A caller that pins the
        # KV split (lvq_tuning.attn_nsplit) is asking for bits that do not follow the batch, and keeps the per-scene pair lists.
        if B >= 3 and not os.environ.get("LVQ_NO_SHARED_SUBTRACT") and not F.get_tuning()["attn_nsplit"]:
            list_src, list_info = ops.bev_shared_lists(row_src, B, n_tiles, hw)
            o = ops.attention_tiled_shared(qp, kv, row_src, list_src, list_info, totals, batch=B, n_heads=h, nq=nq, n_tiles=n_tiles, dh=dh,
                                           scale=1.0 / math.sqrt(dh), totals_k_fp16=totals_k_fp16, tag="ca_attn", k_fp16=k_fp16, stats=stats)
            pair_info = list_info[:B, :2]                       # (tiles, use) per scene, as the pair lists report them
        else:
            pair_src, pair_info = ops.bev_scene_pairs(row_src, B, n_tiles, hw)
            o = ops.attention_tiled_signed(qp, kv, row_src, pair_src, pair_info, totals, batch=B, n_heads=h, nq=nq, n_tiles=n_tiles,
                                           dh=dh, scale=1.0 / math.sqrt(dh), shared_q=True, tag="ca_attn", k_fp16=k_fp16, stats=stats)
        q2 = q2_1.unsqueeze(0).expand(B, nq, d).reshape(B * nq, d)
        y, _ = ops.linear(o, self._w(self.ca.out_proj.weight), self.ca.out_proj.bias, residual=q2, out_f32=True, tag="ca_out_proj")
        self._last_pair_info = pair_info                      # device tensor, read by bench / tests only
        return self._mlp(y)

    def forward_tokens_tiled(self, q2: torch.Tensor, x_rows: BF, kv: torch.Tensor, row_src: torch.Tensor, rows_dev: torch.Tensor, B: int, nq: int,
                             n_tiles: int) -> Tuple[torch.Tensor, BF]:
        """Block over the tiled BEV key stream (csrc/bev_tiles.hip): K|V of the DIRTY rows from x_rows into kv[HW:], every other key
        from the per-model table in kv[:HW].  Plain K / V / P; weights and the query side keep their lo parts in the mixed mode.
        -> (block output, the cross-attention's Q projection BF [B*nq, d]: what the stream guard audits)."""
        d, h = self.d_model, self.n_heads
        dh = d // h
        hw = n_tiles * 64
        q2 = self._self_attn(q2, B, nq)
        if x_rows is not None:
            ops.linear_live_rows(x_rows, self._w(self.ca.in_proj_weight), self.ca.in_proj_bias, rows_dev, (d, 3 * d), tag="ca_kv_proj", out=kv[hw:])
        _, qn = ops.layernorm(q2, self.ca_ln.weight, self.ca_ln.bias, self.ca_ln.eps, self._split())
        _, qp = ops.linear(qn, self._w(self.ca.in_proj_weight), self.ca.in_proj_bias, out_bf=True, w_rows=(0, d), tag="ca_q_proj")
        o = ops.attention_tiled(qp, kv, row_src, batch=B, n_heads=h, nq=nq, n_tiles=n_tiles, dh=dh, scale=1.0 / math.sqrt(dh), tag="ca_attn")
        y, _ = ops.linear(o, self._w(self.ca.out_proj.weight), self.ca.out_proj.bias, residual=q2, out_f32=True, tag="ca_out_proj")
        return self._mlp(y), qp

    def _mlp(self, q2: torch.Tensor) -> torch.Tensor:
        split = self._split()
        _, hn = ops.layernorm(q2, self.mlp_ln.weight, self.mlp_ln.bias, self.mlp_ln.eps, split)
        _, h1 = ops.linear(hn, self._w(self.mlp[0].weight), self.mlp[0].bias, gelu=True, out_bf=True)
        y, _ = ops.linear(h1, self._w(self.mlp[3].weight), self.mlp[3].bias, residual=q2, out_f32=True)
        return y

    # ---- fused short-K/V cross-attention (csrc/cross_fused.hip): the whole `q + ca(ca_ln(q), kv, kv)` in two launches ----
    def _ca_fused_mode(self, B: int, nq: int, nkv: int) -> Optional[bool]:
        """None: not a shape / mode of the fused kernel; else its operand type (True = fp16, False = bf16).  "bf16" runs it on bf16
        operands; the parity-true modes "mixed" / "mixed16" run it on fp16 operands (one MFMA pass at the bf16 rate, 4e-4 from the
        fp32 reference at the headline shape: tools/precision_study_ca.py); "bf16x3" keeps the hi + lo chain."""
        if os.environ.get("LVQ_NO_FUSED_CA") or not ops.ca_fused_ok(B, nq, nkv, self.d_model, self.n_heads):
            return None
        f16 = {"bf16": False, "mixed": True, "mixed16": True}.get(self._mode())
        if f16 and nkv < 128:
            # the fp16 form is parity-true because the softmax averages the per-key roundings: 4e-4 at 196 keys, 8e-4 at 33, 1.4e-3
            # with a single key (tools/precision_study_ca.py) -- short key sets stay on the hi + lo chain
            return None
        return f16

    def _ca_blob(self, f16: bool) -> torch.Tensor:
        params = (self.ca_ln.weight, self.ca_ln.bias, self.ca.in_proj_weight, self.ca.in_proj_bias, self.ca.out_proj.weight, self.ca.out_proj.bias)
        return F.derived(self._wcache, ("ca_fused", f16), params, lambda: ops.ca_fused_pack(*[_f32(p) for p in params], self.n_heads, f16))

    def _cross_attn_fused(self, q2: torch.Tensor, kv: torch.Tensor, B: int, nq: int, f16: bool) -> torch.Tensor:
        out = ops.ca_fused(q2.view(B, nq, self.d_model), kv, self._ca_blob(f16), self.ca_ln.eps, self.n_heads, f16, tag="ca_fused")
        return out.view(B * nq, self.d_model)

    def forward_tokens(self, q2: torch.Tensor, kv_bf: Optional[BF], B: int, nq: int, nkv: int, kv_f32: Optional[torch.Tensor] = None) -> torch.Tensor:
        q2 = self._self_attn(q2, B, nq)
        f16 = self._ca_fused_mode(B, nq, nkv) if kv_f32 is not None else None
        # Inside the whole block the 1e-3 budget is shared with the self-attention, the MLP and whatever produced q (VATLiDAR): the fp16
        # form of the fused kernel (4e-4 on its own) then leaves a 2x margin end to end (5.1e-4 on the bench scene) where the hi + lo
        # chain leaves 9x (1.05e-4) for < 1 % of a pipeline step -- so a parity-true mode takes it here only when asked
        # (`fused_ca_in_block`); the plain-bf16 mode, which makes no parity claim, always does
        if f16 is not None and (not f16 or self.fused_ca_in_block):
            return self._mlp(self._cross_attn_fused(q2, kv_f32, B, nq, f16))
        if kv_bf is None:
            kv_bf = ops.cast(kv_f32.view(B * nkv, self.d_model), self._split())
        if kv_bf[1] is not None and self._stream_plain(nq, nkv, self.d_model // self.n_heads):
            kv_bf = (kv_bf[0], None)                     # mixed mode: the key stream's own rounding averages out
        q2 = self._cross_attn(q2, self.project_kv(kv_bf), B, nq, nkv)
        return self._mlp(q2)

    def forward(self, q: torch.Tensor, kv: torch.Tensor) -> torch.Tensor:
        if self._autograd(q, kv):
            return AG.vat_block(self, q, kv)
        self._guard(q, kv)
        B, nq, d = q.shape
        nkv = kv.shape[1]
        assert d == self.d_model and kv.shape[0] == B and kv.shape[2] == d
        out = self.forward_tokens(_f32(q).view(B * nq, d), None, B, nq, nkv, kv_f32=_f32(kv))
        return out.view(B, nq, d)

    def cross_attention(self, q: torch.Tensor, kv: torch.Tensor) -> torch.Tensor:
        """Only the `q + ca(ca_ln(q), kv, kv)` sub-path (vat_blocks.py:42): the headline kernel sequence."""
        self._guard(q, kv)
        B, nq, d = q.shape
        nkv = kv.shape[1]
        f16 = self._ca_fused_mode(B, nq, nkv)
        if f16 is not None:
            return self._cross_attn_fused(_f32(q).view(B * nq, d), _f32(kv), B, nq, f16).view(B, nq, d)
        kv_bf = ops.cast(_f32(kv).view(B * nkv, d), self._split())
        return self._cross_attn(_f32(q).view(B * nq, d), self.project_kv(kv_bf), B, nq, nkv).view(B, nq, d)


def _lidar_grid_cpu(H: int, W: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """geom [HW,5] = (x, y, r, sin t, cos t), sid [HW] -- input-independent, cached per (H, W, device).
    Evaluated with the reference's exact torch expressions on the host (vat_lidar.py:143-182) so the sector
    ids are bit-identical to the CPU reference, then uploaded once."""
    yv, xv = torch.meshgrid(torch.linspace(-1.0, 1.0, H), torch.linspace(-1.0, 1.0, W), indexing="ij")
    r = torch.clamp((xv ** 2 + yv ** 2).sqrt(), 0.0, 1.0)
    theta = torch.atan2(yv, xv)
    geom = torch.stack((xv, yv, r, torch.sin(theta), torch.cos(theta)), dim=-1).view(H * W, 5)
    ft = theta.view(-1)
    pi = math.pi
    sid = torch.empty(H * W, dtype=torch.long)
    sid[(ft >= pi / 3) & (ft < 2 * pi / 3)] = 0
    sid[(ft >= 0.0) & (ft < pi / 3)] = 1
    sid[(ft >= 2 * pi / 3) & (ft <= pi)] = 2
    sid[(ft >= -2 * pi / 3) & (ft < -pi / 3)] = 3
    sid[(ft >= -pi / 3) & (ft < 0.0)] = 4
    sid[(ft >= -pi) & (ft < -2 * pi / 3)] = 5
    return geom, sid


def _post_head(mod: _HipModule, q2: torch.Tensor, final_ln: nn.LayerNorm, post: nn.Sequential) -> torch.Tensor:
    """final_ln -> LayerNorm -> Linear -> GELU -> (Dropout) -> Linear (vat_lidar.py:295-296, vat_vision.py:214-215)."""
    split = mod._split()
    qf, _ = ops.layernorm(q2, final_ln.weight, final_ln.bias, final_ln.eps, split, want_f32=True, want_bf=False)
    _, hn = ops.layernorm(qf, post[0].weight, post[0].bias, post[0].eps, split)
    _, h1 = ops.linear(hn, mod._w(post[1].weight), post[1].bias, gelu=True, out_bf=True)
    y, _ = ops.linear(h1, mod._w(post[4].weight), post[4].bias, out_f32=True)
    return y


class VATLiDAR(_HipModule):
    """bev [B,C_in,H,W] -> view-aware tokens [B,n_queries,d_model]."""

    def __init__(self, c_in: int, d_model: int, n_queries: int = 576, n_layers: int = 4, n_heads: int = 8,
                 mlp_ratio: float = 4.0, dropout: float = 0.10, post_dropout: float = 0.10):
        super().__init__()
        assert n_queries % NUM_VIEWS == 0, "n_queries must be divisible by NUM_VIEWS (6)."
        self.d_model = d_model
        self.n_queries = n_queries
        self.nq_per_view = n_queries // NUM_VIEWS
        self.refine = nn.Sequential(nn.Conv2d(c_in, c_in, kernel_size=3, padding=1, groups=c_in), nn.GELU())
        self.proj = nn.Conv2d(c_in, d_model, kernel_size=1, bias=True)
        self.norm_tokens = nn.LayerNorm(d_model)
        self.geo_mlp = nn.Sequential(nn.Linear(5, d_model), nn.GELU(), nn.Linear(d_model, d_model))
        self.view_embed = nn.Parameter(torch.zeros(NUM_VIEWS, d_model))
        self.query = nn.Parameter(torch.randn(n_queries, d_model) * 0.02)
        d_ff = int(mlp_ratio * d_model)
        self.blocks = nn.ModuleList([VATBlock(d_model, n_heads, d_ff, dropout) for _ in range(n_layers)])
        self.final_ln = nn.LayerNorm(d_model)
        self.post = nn.Sequential(nn.LayerNorm(d_model), nn.Linear(d_model, d_model), nn.GELU(), nn.Dropout(post_dropout),
                                  nn.Linear(d_model, d_model))
        self._cache: Dict[Tuple[int, int, torch.device], Tuple[torch.Tensor, torch.Tensor]] = {}
        object.__setattr__(self, "_pe_cache", {})
        self.strict_parity = False          # "mixed" modes: audit the key stream of EVERY scene inside every call (one synchronisation, ~4 ms per
                                            # scene at 262 144 keys) and redo a failing call with hi + lo operands
        self.audit_every = 64               # otherwise: every audit_every-th call audits one scene in the background (0 = never)
        if c_in % 8:
            raise ValueError("c_in must be a multiple of 8 (16-byte bf16 operand loads)")

    def _grid(self, H: int, W: int, device: torch.device):
        key = (H, W, device)
        if key not in self._cache:
            geom, sid = _lidar_grid_cpu(H, W)
            self._cache[key] = (geom.to(device), sid.to(device))
        return self._cache[key]

    # ---- what the cached, input-independent values are derived from: each group of parameters is named once ----
    def _pe_params(self) -> List[torch.Tensor]:
        """The positional table's five."""
        return [self.geo_mlp[0].weight, self.geo_mlp[0].bias, self.geo_mlp[2].weight, self.geo_mlp[2].bias, self.view_embed]

    def _table_params(self) -> List[torch.Tensor]:
        """Everything the K|V table of the empty scene reads: refine conv, token projection and LayerNorm, the positional table (eleven
        tensors) and every block's K|V projection."""
        params = [self.refine[0].weight, self.refine[0].bias, self.proj.weight, self.proj.bias, self.norm_tokens.weight, self.norm_tokens.bias]
        params += self._pe_params()
        for blk in self.blocks:
            params += [blk.ca.in_proj_weight, blk.ca.in_proj_bias]
        return params

    def _query_params(self, blk: "VATBlock") -> List[torch.Tensor]:
        """Everything a block's shared query side reads: the learned queries and the block's self-attention and Q projection (twelve)."""
        return [self.query, self.view_embed, blk.sa_ln.weight, blk.sa_ln.bias, blk.sa.in_proj_weight, blk.sa.in_proj_bias, blk.sa.out_proj.weight,
                blk.sa.out_proj.bias, blk.ca_ln.weight, blk.ca_ln.bias, blk.ca.in_proj_weight, blk.ca.in_proj_bias]

    def _pe_table(self, H: int, W: int, device) -> torch.Tensor:
        """geo_mlp(geom) + view_embed[sid]: [HW, d] fp32, input-independent -> cached per weights version."""
        split = self._split()

        def build():
            geom, sid = self._grid(H, W, device)
            g8 = torch.nn.functional.pad(geom, (0, 3)).contiguous()            # K = 5 -> 8 (zero columns)
            _, h1 = ops.linear(ops.cast(g8, split), self._w(self.geo_mlp[0].weight, pad_k=8), self.geo_mlp[0].bias, gelu=True,
                               out_bf=True)
            ve = self.view_embed.detach().float()[sid].contiguous()            # gather of a 6-row table (index plumbing)
            return ops.linear(h1, self._w(self.geo_mlp[2].weight), self.geo_mlp[2].bias, residual=ve, out_f32=True)[0]
        return F.derived(self._pe_cache, (H, W, device), self._pe_params(), build, (split,))

    def bev_tokens(self, bev: torch.Tensor) -> BF:
        """vat_lidar.py:212-248: refine -> proj -> LayerNorm -> + geo PE + view embed; BF [B*HW, d]."""
        B, C, H, W = bev.shape
        split = self._split()
        t = ops.dwconv3x3_gelu(_f32(bev), self.refine[0].weight.detach().reshape(C, 9).contiguous(), self.refine[0].bias, split)
        pe = self._pe_table(H, W, bev.device)
        return self._tokens_to_model(t, H, W, bev.device)

    def _tokens_to_model(self, t: BF, H: int, W: int, dev) -> BF:
        """conv tokens t [B*HW, C] -> BEV tokens x [B*HW, d] = LayerNorm(proj(t)) + positional table (vat_lidar.py:222-248).
        In mixed mode with a long key stream x leaves plain (its rounding is independent per key) from split t and W_proj."""
        pe = self._pe_table(H, W, dev)
        C = t[0].shape[1]
        blk = self.blocks[0]
        plain_x = self._stream_plain(self.n_queries, H * W, blk.d_model // blk.n_heads)
        if ops.linear_ln_supported(self.d_model, C):
            # 1x1 conv + LayerNorm + positional table in one row-complete kernel: no fp32 [B*HW, d] round trip
            return ops.linear_ln(t, self._w(self.proj.weight), self.proj.bias, self.norm_tokens.weight, self.norm_tokens.bias,
                                 self.norm_tokens.eps, post=pe, tag="bev_proj_ln", out_lo=not plain_x)
        x32, _ = ops.linear(t, self._w(self.proj.weight), self.proj.bias, out_f32=True)
        _, x = ops.layernorm(x32, self.norm_tokens.weight, self.norm_tokens.bias, self.norm_tokens.eps, self._split() and not plain_x, post=pe)
        return x

    # ---- sparse (tiled) key stream: csrc/bev_tiles.hip ------------------------------------------------------------------
    def _tiled_route_ok(self, C: int, H: int, W: int) -> bool:
        """Pillar route with 8 x 8-cell key tiles: 64-channel pillars, grid sides multiples of 8, a width the fused token kernel
        builds, head_dim 64 and a key stream long enough for the long-stream attention kernel; plain or mixed operands (bf16x3
        keeps lo parts of K / V, which the tiled kernels do not carry)."""
        blk = self.blocks[0]
        return (C == 64 and H % 8 == 0 and W % 8 == 0 and self.d_model in (256, 512, 768, 1024) and blk.d_model // blk.n_heads == 64
                and self._mode() in ("bf16", "mixed", "mixed16") and ops.attention_stream_ok(self.n_queries, H * W, 64)
                and not os.environ.get("LVQ_NO_TILED_STREAM"))

    def _sparse_route_ok(self, C: int, H: int, W: int) -> bool:
        """_tiled_route_ok and whole groups of four tiles (the row granularity of the tile kernels)."""
        return self._tiled_route_ok(C, H, W) and not (H // 8) * (W // 8) * 64 % 256

    def _pe_tiled(self, H: int, W: int, dev) -> torch.Tensor:
        """The positional table with its rows in the key order of the tiled stream: tile t (8 x 8 cells) major, then piece p = 2 (y >> 1)
        + (x >> 2) (2 x 4 cells), then 4 (y & 1) + (x & 3) inside the piece -- a permutation of _pe_table."""

        def build():
            pe = self._pe_table(H, W, dev)
            return pe.view(H // 8, 4, 2, W // 8, 2, 4, pe.shape[1]).permute(0, 3, 1, 4, 2, 5, 6).reshape(H * W, -1).contiguous()
        return F.derived(self._pe_cache, ("tiled", H, W, dev), self._pe_params(), build, (self._split(),))

    def _tile_tokens(self, feat, idx, live, dirty, counts, cap_rows, batch, H, W) -> BF:
        C = feat.shape[1]
        return ops.bev_tile_tokens(feat, idx, live, dirty, counts, cap_rows, batch, H, W, self.refine[0].weight.detach().reshape(C, 9).contiguous(),
                                   self.refine[0].bias, self._w(self.proj.weight), self.proj.bias, self.norm_tokens.weight, self.norm_tokens.bias,
                                   self.norm_tokens.eps, self._pe_tiled(H, W, feat.device), out_lo=False, tag="bev_proj_ln")

    def _kv_fold(self, C: int, H: int, W: int, dev):
        """LayerNorm and the K|V projection folded onto the 64-channel conv token (csrc/bev_tiles.hip: k_tile_kv; exact algebra):
            K|V = W_kv (LN(Wp t + bp) + PE) + b_kv = rstd (M t + m0) + T[key],  rstd = 1 / sqrt((|R t + r0|^2 + c0) / d + eps)
        -> (R BF [64, 64], r0 [64], c0, per layer (M BF [2d, 64], m0 [2d], T [HW, 2d] fp32 in tile-major key order)), cached per weights
        version and precision mode.  The small factors are folded in fp64 (model-load-time plumbing, like folding a BatchNorm); the
        table T runs through lvq_gemm_bf16 in the mode's operand form."""
        t16 = bool(os.environ.get("LVQ_KV_T_FP16")) and not os.environ.get("LVQ_KV_ONE_LAUNCH")    # opt-in fp16 table (two-launch form only)

        def build():
            split = self._split()
            d = self.d_model
            f64 = lambda p: p.detach().to(device="cpu", dtype=torch.float64)      # the small factors: host fp64 (a 768 x 65 QR, two thin products)
            wp, bp = f64(self.proj.weight).view(d, C), f64(self.proj.bias)
            wc, bc = wp - wp.mean(0, keepdim=True), bp - bp.mean()
            rr = torch.linalg.qr(torch.cat((wc, bc[:, None]), 1), mode="r").R          # [C + 1, C + 1]: |Wc t + bc|^2 = |R [t; 1]|^2
            r_bf = ops.cast(rr[:C, :C].float().contiguous().to(dev), split)
            r0 = rr[:C, C].float().contiguous().to(dev)
            c0 = float(rr[C, C] ** 2)
            gam, bet = f64(self.norm_tokens.weight), self.norm_tokens.bias.detach().float().view(1, d).contiguous()
            a_pe = ops.cast(ops.scale_add_rows(self._pe_tiled(H, W, dev), bet), split)  # beta + PE[key], the A operand of the table GEMM
            # |LayerNorm(y)_n| <= sqrt(d) whatever the input, so |x_n| <= sqrt(d) |gamma_n| + |beta_n| + max_key |PE_n| and every K entry of
            # layer 0 is bounded by its weight row's L1 product with that: the static guarantee behind the fp16 K half of "mixed16"
            xmax = (math.sqrt(d) * gam.abs() + f64(self.norm_tokens.bias).abs() + self._pe_tiled(H, W, dev).abs().amax(0).double().cpu())
            wk0, bk0 = f64(self.blocks[0].ca.in_proj_weight)[d:2 * d], f64(self.blocks[0].ca.in_proj_bias)[d:2 * d]
            k_bound = float((wk0.abs() @ xmax + bk0.abs()).max())
            layers = []
            for blk in self.blocks:
                blk.precision = self.precision
                wkv = f64(blk.ca.in_proj_weight)[d:]
                m_bf = ops.cast((wkv @ (gam[:, None] * wc)).float().contiguous().to(dev), split)
                m0 = (wkv @ (gam * bc)).float().contiguous().to(dev)
                t_tab, _ = ops.linear(a_pe, blk._w(blk.ca.in_proj_weight), blk.ca.in_proj_bias, out_f32=True, w_rows=(d, 3 * d))
                # the table as fp16 when its values fit (checked once, here): its 2^-12 rounding disappears under the bf16 rounding of the
                # rows, and the kernel's largest read stream halves (two-launch form only; dtype conversion = plumbing)
                # LVQ_KV_T_FP16=1: the table as IEEE fp16 (values checked here) -- half the bytes of k_kv_rows' largest read stream, 4.5 -> 3.8 ms,
                # +4 % tokens/s.  Opt-in, because it is not free: rounding T to 11 bits moves the fused tokens by 1.4e-4 (1.04e-4 -> 2.4e-4 against
                # the oracle; linear in the rounding -- bf16 would cost 1.5e-3 -- and mostly through the V half: DESIGN 3.3)
                if t16 and float(t_tab.abs().max()) < 3.0e4:
                    t_tab = t_tab.to(torch.float16)
                layers.append((m_bf, m0, t_tab))
            return r_bf, r0, c0, layers, k_bound
        return F.derived(self._pe_cache, ("kv_fold", H, W, dev), self._table_params(), build, (self._mode(), t16))

    def _tile_kv(self, li: int, feat, idx, live, dirty, counts, cap_rows, batch, H, W, out, k_fp16: bool = False) -> None:
        C = feat.shape[1]
        r_bf, r0, c0, layers, _ = self._kv_fold(C, H, W, feat.device)
        m_bf, m0, t_tab = layers[li]
        ops.bev_tile_kv(feat, idx, live, dirty, counts, cap_rows, batch, H, W, self.refine[0].weight.detach().reshape(C, 9).contiguous(),
                        self.refine[0].bias, m_bf, m0, r_bf, r0, c0, self.d_model, self.norm_tokens.eps, t_tab, out, tag="bev_kv",
                        split_launch=k_fp16 or not os.environ.get("LVQ_KV_ONE_LAUNCH"), k_fp16=k_fp16)

    def _kv_buffers(self, C: int, H: int, W: int, dev, batch: int, k16: bool = False) -> List[torch.Tensor]:
        """Per layer ONE K|V buffer [HW + batch*HW, 2d] bf16.  Rows 0 .. HW-1: the per-model TABLE = K|V of the EMPTY scene by the same
        kernel that serves the dirty rows (every cell forced dirty; key order = tile-major), cached per weights version and precision
        mode -- input-independent like the positional table.  Rows HW ..: the step's computed rows (capacity for `batch` scenes)."""
        fused = not os.environ.get("LVQ_NO_FUSED_KV")
        key = ("kv_buffer", H, W, dev)
        hw, d = H * W, self.d_model
        rows = hw + batch * hw

        def build():
            # a new table: whatever was derived from the old one (block 0's softmax totals) goes with it -- content identity is the
            # version tuple, never the buffer address (a freed block can come back from the allocator with other contents)
            self._pe_cache.pop(("signed_totals", H, W, dev), None)
            idx = torch.full((1, H, W), -1, dtype=torch.int32, device=dev)
            live, dirty, src, counts = ops.bev_tiles(idx, 1, H, W, dev, 0, force_all=True)
            feat = torch.zeros((1, C), dtype=torch.float32, device=dev)
            x = None if fused else self._tile_tokens(feat, idx, live, dirty, counts, hw, 1, H, W)
            bufs = []
            for li, blk in enumerate(self.blocks):
                blk.precision = self.precision
                buf = torch.empty((rows, 2 * d), dtype=torch.bfloat16, device=dev)
                if fused:
                    self._tile_kv(li, feat, idx, live, dirty, counts, hw, 1, H, W, buf[:hw], k_fp16=k16 and li == 0)
                else:
                    ops.linear_live_rows(x, blk._w(blk.ca.in_proj_weight), blk.ca.in_proj_bias, counts[2:], (d, 3 * d), out=buf[:hw])
                bufs.append(buf)
            return bufs
        bufs = F.derived(self._pe_cache, key, self._table_params(), build,
                         (self._mode(), fused, k16, bool(os.environ.get("LVQ_KV_ONE_LAUNCH")), bool(os.environ.get("LVQ_KV_T_FP16"))))
        if bufs[0].shape[0] < rows:                             # a larger batch: new buffers under the unchanged version, the table rows copied over
            grown = [torch.empty((rows, 2 * d), dtype=torch.bfloat16, device=dev) for _ in bufs]
            for buf, old in zip(grown, bufs):
                buf[:hw].copy_(old[:hw])
            self._pe_cache[key] = (self._pe_cache[key][0], grown)
            return grown
        return bufs

    def _query_side(self, blk: "VATBlock", dev) -> Tuple[torch.Tensor, BF]:
        """Block 0's shared_query_side on the learned queries: every input is a parameter, so (q after self-attention, Q projection) is
        computed once per weights version, precision mode and device (about eight dependent launches off every step).  Same kernels on the
        same inputs give the same bits, so the cached pair is what a fresh call would return and the cached `totals` stay its totals.
        Both tensors are read-only downstream (residual / attention operands, the guard's audit)."""
        return F.derived(self._pe_cache, ("query_side", blk._mode(), dev), self._query_params(blk),
                         lambda: blk.shared_query_side(self._queries(1), self.n_queries))

    def _q16_ok(self, blk: "VATBlock", qp: BF) -> bool:
        """mixed16: the scaled queries of block 0 fit fp16 (they depend on the weights only: checked once per weights version)."""
        dh = blk.d_model // blk.n_heads
        return F.derived(self._pe_cache, "q16_ok", self._query_params(blk),
                         lambda: float(ops.to_f32(qp).abs().max()) * (1.0 / math.sqrt(dh)) * 1.4426950408889634 < 3.0e4, (self._mode(),))

    # ---- guard of the plain-bf16 key stream (the "mixed" modes): DESIGN 3.3 ----
    STREAM_GUARD_MAX = 0.5     # max over (head, query) of (1 + max |score|) / sqrt(N_eff); tools/mixed_guard_study.py: 0.04 on the bench model
                               # (error 7e-5), 0.13 -> 2e-4, 0.38 -> 3.7e-4, 1.1 -> 9e-4, 4 -> 1.7e-3, 12 -> 4e-3 (tolerance 1e-3)

    def stream_guard(self, C: int, H: int, W: int, dev) -> float:
        """Per-model half of the guard: the statistic of block 0's (scene-independent) cross-attention queries over the keys of the
        K|V table = the EMPTY scene's keys, 70-100 % of every scene's keys.  Plain bf16 K / V / P are parity-true because their per-key
        roundings average out over the keys that carry the softmax mass; when the model's attention is peaked (few keys carry it, large
        scores) they do not, and the modes that rely on it run the hi + lo route instead (forward_pillars).  Once per weights version."""
        blk = self.blocks[0]

        def build():
            keep = self.precision
            try:
                self.precision = "mixed"                       # the statistic is taken on the stream it guards: the plain table of the mixed mode
                blk.precision = "mixed"
                _, qp = self._query_side(blk, dev)             # cached under the mode forced here, not the caller's
                table = self._kv_buffers(C, H, W, dev, 1, False)[0]
                dh = blk.d_model // blk.n_heads
                return float(ops.stream_guard(qp[0], table[:H * W], blk.n_heads, 1.0 / math.sqrt(dh)).max())
            finally:
                self.precision = keep
                blk.precision = keep
        return F.derived(self._pe_cache, ("stream_guard", H, W, dev), self._query_params(blk) + self._table_params(), build)

    def guard_counters(self) -> Tuple[int, int, float]:
        """Per-launch half of the guard, accumulated since the module was created (reads the device: a synchronisation): (rows whose
        softmax mass moved onto the scene's own keys -- row sum > 1.5x the table's; not covered by the per-model statistic --, (scene, head)
        pairs re-run by the cancellation check of the signed stream, largest row sum / table row sum seen)."""
        st = getattr(self, "_guard_stats", None)
        if st is None:
            return (0, 0, 0.0)
        a, b, c, _ = st.cpu().tolist()
        return int(a), int(b), float(torch.tensor([c], dtype=torch.int32).view(torch.float32))

    def _audit_scene(self, qp_hi: torch.Tensor, table: torch.Tensor, src: torch.Tensor, scene: int, n_keys: int, k16: bool = False) -> torch.Tensor:
        """Per-scene half of the guard: the statistic of lvq_stream_guard on the ACTUAL key stream of one scene for one block (qp_hi [nq, d]:
        that block's queries for this scene; its K|V buffer's computed rows and the table rows of the clean cells, gathered through row_src)
        -> 0-d device tensor max(g).  ~4 ms at 262 144 keys: run on a sample of the scenes (audit_every) or on all of them (first call of a
        weights version, strict_parity)."""
        blk = self.blocks[0]
        d = blk.d_model
        rows = src.view(-1, n_keys)[scene].long()
        k_scene = table[:, :d].index_select(0, rows)                      # gather copy (plumbing): this scene's K rows in stream order
        if k16:                                                           # "mixed16": the K half holds IEEE fp16 bit patterns
            k_scene = k_scene.view(torch.float16).to(torch.bfloat16)
        return ops.stream_guard(qp_hi, k_scene, blk.n_heads, 1.0 / math.sqrt(d // blk.n_heads)).max()

    def _audit(self, qps: List[torch.Tensor], kvs: List[torch.Tensor], src: torch.Tensor, scenes, n_keys: int, k16: bool) -> torch.Tensor:
        """_audit_scene over the given scenes and EVERY block: qps[li] = block li's Q projection (hi part), [nq, d] when shared by all scenes
        (block 0 of the signed stream) else [batch * nq, d] -> 0-d device tensor, the largest statistic."""
        nq = self.n_queries
        g = [self._audit_scene(q if q.shape[0] == nq else q[b * nq:(b + 1) * nq], kvs[li], src, b, n_keys, k16 and li == 0)
             for li, q in enumerate(qps) for b in scenes]
        return torch.stack(g).max()

    def _guard_poll(self) -> bool:
        """True when an audit whose read-back has completed exceeded the threshold (no synchronisation: the answer lags by a call or two)."""
        pend = getattr(self, "_guard_pending", None)
        if pend is not None and pend[0].query():
            object.__setattr__(self, "_guard_pending", None)
            return float(pend[1][0]) > self.STREAM_GUARD_MAX
        return False

    def _guard_submit(self, g: torch.Tensor):
        """Start the read-back of an audit result (pinned host memory, no wait); at most one in flight."""
        if getattr(self, "_guard_pending", None) is not None:
            return
        host = torch.empty(1, dtype=torch.float32, pin_memory=True)
        host.copy_(g.reshape(1), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(g.device))
        object.__setattr__(self, "_guard_pending", (ev, host))

    def _signed_totals(self, blk: "VATBlock", qp: BF, kv: torch.Tensor, H: int, W: int, dev, k_fp16: bool = False) -> torch.Tensor:
        """Softmax sums of block 0's (scene-independent) cross-attention queries over ALL keys of the K|V table -> fp32
        [heads, nq, 66]; input-independent like the table itself, cached per weights version.  `qp` is this step's Q projection:
        the cached totals belong to exactly these bits as long as the version key is unchanged."""
        # the table side of the totals: the version tuple of the K|V buffers they were computed from (all table-side parameters,
        # precision mode, fused / k16 / route flags -- _kv_buffers), not the buffer's address
        kv_hit = self._pe_cache.get(("kv_buffer", H, W, dev))
        kv_ver = kv_hit[0] if kv_hit is not None and any(b is kv for b in kv_hit[1]) else ("unversioned",) + F.version_of((kv,))
        dh = blk.d_model // blk.n_heads
        q16 = bool(os.environ.get("LVQ_TOTALS_Q16"))
        # mixed16: the totals keep the full query (fp16 hi + lo against the fp16 table keys, k_fp16 = 2) unless LVQ_TOTALS_Q16 asks for the
        # once-rounded query of the per-scene streams
        return F.derived(self._pe_cache, ("signed_totals", H, W, dev), self._query_params(blk),
                         lambda: ops.attention_stream_totals(qp, kv[:H * W], n_heads=blk.n_heads, nq=self.n_queries, nkv=H * W, dh=dh,
                                                             scale=1.0 / math.sqrt(dh), k_fp16=(1 if q16 else 2) if k_fp16 else 0),
                         (self._mode(), kv_ver, k_fp16, q16))

    def forward_pillars(self, pillar_features: torch.Tensor, coords_bzyx: torch.Tensor, n_live: Optional[torch.Tensor],
                        batch: int, H: int, W: int, all_tiles_live: bool = False) -> torch.Tensor:
        """Same result as forward(PointPillarScatter(pillars)) without the dense BEV canvas.  Default route (shapes of
        _tiled_route_ok): the sparse key stream of csrc/bev_tiles.hip -- tokens and K|V only for the tiles that hold a pillar in
        their halo, the rest from the per-model table; `all_tiles_live=True` computes every tile per scene (the dense comparator:
        the two are bit-identical).  Other shapes: scatter + refine conv as one sparse gather (ops.pillar_dwconv3x3_gelu)."""
        self._guard(pillar_features)
        C = pillar_features.shape[1]
        dev = pillar_features.device
        feat = _f32(pillar_features)
        tiled = self._sparse_route_ok(C, H, W)
        guarded = tiled and self._mode() in ("mixed", "mixed16") and not os.environ.get("LVQ_NO_STREAM_GUARD")
        if guarded:
            # The plain-bf16 key stream is parity-true only while the softmax mass is spread over many keys.  Two checks of the
            # same statistic (lvq_stream_guard), both structural: (1) once per weights version, the model's own queries over the table keys
            # (the empty scene: 70-100 % of every scene's keys); (2) an audit of the ACTUAL key stream of every block -- every scene of the
            # first call of a weights version, with the call redone on the spot if it fails (and so of every call with strict_parity); then
            # every audit_every-th call one scene (results are read back without synchronisation and trip the module a call or two later).
            # A model / scene stream that fails runs hi + lo operands everywhere instead.
            ver = self._guard_version()
            if getattr(self, "_guard_ver", None) != ver:         # new weights: audited afresh, nothing read back under the old ones applies
                object.__setattr__(self, "_guard_ver", ver)
                object.__setattr__(self, "_guard_calls", 0)
                object.__setattr__(self, "_guard_pending", None)
            tripped = getattr(self, "_guard_tripped", None) == ver
            if not tripped and self._guard_poll():
                object.__setattr__(self, "_guard_tripped", ver)
                tripped = True
            if tripped or self.stream_guard(C, H, W, dev) > self.STREAM_GUARD_MAX:
                return self._forward_pillars_hilo(pillar_features, coords_bzyx, n_live, batch, H, W, all_tiles_live)
        if not tiled:
            t = ops.pillar_dwconv3x3_gelu(feat, coords_bzyx, n_live, batch, H, W,
                                          self.refine[0].weight.detach().reshape(C, 9).contiguous(), self.refine[0].bias, self._split())
            return self._decode(self._tokens_to_model(t, H, W, dev), batch, H, W)
        nt = (H // 8) * (W // 8)
        fused = not os.environ.get("LVQ_NO_FUSED_KV")          # K|V straight from the conv token (k_tile_kv) vs tokens -> K|V GEMM
        signed = not all_tiles_live and not os.environ.get("LVQ_NO_SIGNED_STREAM")
        q2_1 = qp = None
        k16 = False
        if signed:
            # block 0: the queries are the same for every scene -> query side once, attention over the dirty rows only
            self.blocks[0].precision = self.precision
            q2_1, qp = self._query_side(self.blocks[0], dev)
            # "mixed16": fp16 Q K^T in block 0 when K (static bound from the fold) and the scaled Q provably fit fp16
            k16 = (self._mode() == "mixed16" and fused and self._kv_fold(C, H, W, dev)[4] < 3.0e4 and self._q16_ok(self.blocks[0], qp))
        kvs = self._kv_buffers(C, H, W, dev, batch, k16)
        idx = ops.pillar_index_map(coords_bzyx, n_live, batch, H, W)
        live, dirty, src, counts = ops.bev_tiles(idx, batch, H, W, dev, H * W, force_all=all_tiles_live)
        x_live = None if fused else self._tile_tokens(feat, idx, live, dirty, counts, batch * nt * 64, batch, H, W)
        q2 = None if signed else self._queries(batch)
        qps = []                                               # every block's Q projection (hi part): the guard's audit
        for li, (blk, table) in enumerate(zip(self.blocks, kvs)):
            blk.precision = self.precision
            if fused:
                self._tile_kv(li, feat, idx, live, dirty, counts, batch * nt * 64, batch, H, W, table[H * W:], k_fp16=k16 and li == 0)
            if li == 0 and signed:
                totals = self._signed_totals(blk, qp, table, H, W, dev, k_fp16=k16)
                if getattr(self, "_guard_stats", None) is None or self._guard_stats.device != dev:
                    object.__setattr__(self, "_guard_stats", torch.zeros(4, dtype=torch.int32, device=dev))
                q2 = blk.forward_tokens_tiled_signed(q2_1, qp, totals, x_live, table, src, counts[2:], batch, self.n_queries, nt, k_fp16=k16,
                                                     stats=self._guard_stats,
                                                     totals_k_fp16=(1 if os.environ.get("LVQ_TOTALS_Q16") else 2) if k16 else 0)
                qps.append(qp[0])
            else:
                q2, qp_l = blk.forward_tokens_tiled(q2, x_live, table, src, counts[2:], batch, self.n_queries, nt)
                qps.append(qp_l[0])
        self._last_tile_counts = counts                       # device tensor (live pieces, their rows, dirty rows): read by bench / tests only
        if guarded:
            calls = self._guard_calls
            object.__setattr__(self, "_guard_calls", calls + 1)
            if self.strict_parity or calls == 0:
                g = self._audit(qps, kvs, src, range(batch), H * W, k16)
                if float(g) > self.STREAM_GUARD_MAX:             # synchronises: this very call is redone with hi + lo operands
                    object.__setattr__(self, "_guard_tripped", self._guard_version())
                    return self._forward_pillars_hilo(pillar_features, coords_bzyx, n_live, batch, H, W, all_tiles_live)
            elif self.audit_every and calls % self.audit_every == 0:
                self._guard_submit(self._audit(qps, kvs, src, [(calls // self.audit_every) % batch], H * W, k16))
        return _post_head(self, q2, self.final_ln, self.post).view(batch, self.n_queries, self.d_model)

    def _guard_version(self):
        return F.version_of(self.parameters())

    def _forward_pillars_hilo(self, pillar_features, coords_bzyx, n_live, batch, H, W, all_tiles_live):
        keep = self.precision
        self.precision = "bf16x3"
        try:
            return self.forward_pillars(pillar_features, coords_bzyx, n_live, batch, H, W, all_tiles_live)
        finally:
            self.precision = keep

    def forward(self, bev: torch.Tensor) -> torch.Tensor:
        if self._autograd(bev):
            return AG.vat_lidar(self, bev)
        self._guard(bev)
        B, C, H, W = bev.shape
        if self._sparse_route_ok(C, H, W) and not os.environ.get("LVQ_NO_DENSE_SPARSE"):
            # the reference's own entry point on the sparse key stream: an all-zero cell of the canvas is exactly an absent pillar (the refine
            # conv sees zeros there either way), and LiDAR canvases are mostly empty -- occupied cells out, then the pillar route
            feats, coords, n_cells = ops.bev_occupied_cells(_f32(bev))
            return self.forward_pillars(feats, coords, n_cells, B, H, W)
        x = self.bev_tokens(bev)
        return self._decode(x, B, H, W)

    def _queries(self, B: int) -> torch.Tensor:
        """queries + per-view embedding (vat_lidar.py:259-270), broadcast over the batch -> [B * nq, d] fp32."""
        ve = self.view_embed.detach().float().repeat_interleave(self.nq_per_view, dim=0).contiguous()
        q0 = ops.scale_add_rows(self.query.detach().float().contiguous(), ve)
        return q0.unsqueeze(0).expand(B, -1, -1).contiguous().view(B * self.n_queries, self.d_model)

    def _decode(self, x: BF, B: int, H: int, W: int) -> torch.Tensor:
        q2 = self._queries(B)
        for blk in self.blocks:
            blk.precision = self.precision
            q2 = blk.forward_tokens(q2, x, B, self.n_queries, H * W)
        return _post_head(self, q2, self.final_ln, self.post).view(B, self.n_queries, self.d_model)


class VATVision(_HipModule):
    """[B, n_input_tokens, d_in] -> [B, n_input_tokens/compression_factor, d_model]."""

    def __init__(self, d_in: int, d_model: int, n_input_tokens: int = 1536, compression_factor: int = 2, n_layers: int = 4,
                 n_heads: int = 8, mlp_ratio: float = 4.0, dropout: float = 0.10, post_dropout: float = 0.10,
                 use_per_view_query: bool = False, strict_per_view: bool = False):
        super().__init__()
        assert n_input_tokens % compression_factor == 0, \
            f"n_input_tokens ({n_input_tokens}) must be divisible by compression_factor ({compression_factor})"
        self.d_in, self.d_model = d_in, d_model
        self.n_input_tokens, self.compression_factor = n_input_tokens, compression_factor
        self.n_queries = n_input_tokens // compression_factor
        feasible = NUM_VIEWS > 0 and self.n_queries >= NUM_VIEWS and self.n_queries % NUM_VIEWS == 0
        if use_per_view_query and not feasible:
            if strict_per_view:
                raise ValueError(f"Per-view queries requested but not feasible: n_queries={self.n_queries}, NUM_VIEWS={NUM_VIEWS}. "
                                 f"Either increase n_queries to be divisible by {NUM_VIEWS}, or set use_per_view_query=False, "
                                 f"or set strict_per_view=False for auto-disable.")
            print("[VATVision] Warning: use_per_view_query=True requested but not feasible:")
            print(f"             n_queries={self.n_queries}, NUM_VIEWS={NUM_VIEWS}")
            print("             Automatically disabling per-view queries.")
            use_per_view_query = False
        self.use_per_view_query = use_per_view_query
        self.nq_per_view = self.n_queries // NUM_VIEWS if use_per_view_query else 0
        self.query = nn.Parameter(torch.randn(self.n_queries, d_in) * 0.02)
        if self.use_per_view_query:
            self.view_query_embed = nn.Parameter(torch.zeros(NUM_VIEWS, d_in))
            nn.init.trunc_normal_(self.view_query_embed, std=0.02)
        else:
            self.view_query_embed = None
        d_ff = int(mlp_ratio * d_in)
        self.blocks = nn.ModuleList([VATBlock(d_in, n_heads, d_ff, dropout) for _ in range(n_layers)])
        self.final_ln = nn.LayerNorm(d_in)
        self.post = nn.Sequential(nn.LayerNorm(d_in), nn.Linear(d_in, d_in), nn.GELU(), nn.Dropout(post_dropout),
                                  nn.Linear(d_in, d_in))
        self.proj = nn.Sequential(nn.LayerNorm(d_in), nn.Linear(d_in, d_model), nn.GELU(), nn.Dropout(dropout),
                                  nn.Linear(d_model, d_model), nn.LayerNorm(d_model))

    def forward(self, kv_tokens: torch.Tensor) -> torch.Tensor:
        B, N, D = kv_tokens.shape
        assert N == self.n_input_tokens, f"Expected {self.n_input_tokens} input tokens, got {N}"
        assert D == self.d_in, f"Expected d_in={self.d_in}, got {D}"
        if self._autograd(kv_tokens):
            return AG.vat_vision(self, kv_tokens)
        self._guard(kv_tokens)
        split = self._split()
        kv = ops.cast(_f32(kv_tokens).view(B * N, D), split)
        q0 = self.query.detach().float().contiguous()
        if self.use_per_view_query and self.nq_per_view > 0:
            q0 = ops.scale_add_rows(q0, self.view_query_embed.detach().float().repeat_interleave(self.nq_per_view, dim=0).contiguous())
        q2 = q0.unsqueeze(0).expand(B, -1, -1).contiguous().view(B * self.n_queries, D)
        for blk in self.blocks:
            blk.precision = self.precision
            q2 = blk.forward_tokens(q2, kv, B, self.n_queries, N)
        q2 = _post_head(self, q2, self.final_ln, self.post)
        _, hn = ops.layernorm(q2, self.proj[0].weight, self.proj[0].bias, self.proj[0].eps, split)
        _, h1 = ops.linear(hn, self._w(self.proj[1].weight), self.proj[1].bias, gelu=True, out_bf=True)
        y, _ = ops.linear(h1, self._w(self.proj[4].weight), self.proj[4].bias, out_f32=True)
        out, _ = ops.layernorm(y, self.proj[5].weight, self.proj[5].bias, self.proj[5].eps, split, want_f32=True, want_bf=False)
        return out.view(B, self.n_queries, self.d_model)


class VisionAdapter(_HipModule):
    """6 x [HW, d_in] -> [6*HW, d_in]: LayerNorm(t + view_embed[v]) per view, concatenated (eval: no dropout)."""

    def __init__(self, d_in: int, dropout: float = 0.10):
        super().__init__()
        self.d_in = d_in
        self.num_views = len(CAM_VIEWS)
        self.norm = nn.LayerNorm(d_in)
        self.dropout = nn.Dropout(dropout)
        self.view_embed = nn.Parameter(torch.zeros(self.num_views, d_in), requires_grad=True)
        nn.init.trunc_normal_(self.view_embed, std=0.02)

    def forward(self, views_tokens: List[torch.Tensor]) -> torch.Tensor:
        if len(views_tokens) != self.num_views:
            raise ValueError(f"Expected {self.num_views} views in order {CAM_VIEWS}, got {len(views_tokens)}")
        hw = None
        for v_idx, t in enumerate(views_tokens):
            if t.dim() != 2:
                raise ValueError(f"Expected tensor of shape [HW, d_in] for view {v_idx}, got shape {tuple(t.shape)}")
            if hw is None:
                hw = t.shape[0]
            elif t.shape[0] != hw:
                raise ValueError(f"All views must have same HW. Got {hw} and {t.shape[0]}.")
        if self._autograd(*views_tokens):
            return AG.vision_adapter(self, views_tokens)
        self._guard(*views_tokens)
        x = torch.cat([_f32(t) for t in views_tokens], dim=0)            # view-major rows: group v = rows v*hw..(v+1)*hw
        out, _ = ops.layernorm(x, self.norm.weight, self.norm.bias, self.norm.eps, False, want_f32=True, want_bf=False,
                               add=self.view_embed.detach().float().contiguous(), add_group=hw)
        return out


def sdp_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attn_mask: Optional[torch.Tensor] = None,
                  precision: Optional[str] = None) -> torch.Tensor:
    """[B,H,S,D] x3 (+ additive mask/bias [B,H,S,S]) -> [B,H,S,D] (deepencoder/clip_sdpa.py:50-66)."""
    F.require_cuda(q, k, v, attn_mask)
    B, H, S, D = q.shape
    Sk = k.shape[2]
    split = (precision or ops.default_precision()) == "bf16x3"
    qb, kb, vb = (ops.cast(_f32(t).view(B * H * t.shape[2], D), split) for t in (q, k, v))
    bias = None if attn_mask is None else _f32(attn_mask.expand(B, H, S, Sk))
    # output addressed as [B, S, H*D] by the ABI; request [B,H,S,D] through the strides instead
    oh, ol = ops._bf_empty((B * H * S, D), q.device, split)
    L = F.lib()
    nbytes = L.lvq_attention_workspace_bytes(B, H, S, Sk, D, 3 if split else 1)
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=q.device)
    rc = L.lvq_attention_bf16(F.ptr(qb[0]), F.ptr(qb[1]), F.ptr(kb[0]), F.ptr(kb[1]), F.ptr(vb[0]), F.ptr(vb[1]), F.ptr(bias),
                              B, H, H, S, Sk, D,
                              H * S * D, D, S * D, H * Sk * D, D, Sk * D,
                              H * Sk * D, D, Sk * D, H * S * D, D, S * D,
                              1.0 / math.sqrt(D), 0, F.ptr(oh), F.ptr(ol), F.ptr(ws), ws.numel(),
                              F.stream_ptr(q.device))
    F.check(rc, "lvq_attention_bf16")
    return ops.to_f32((oh, ol)).view(B, H, S, D)


class MlpProjectorLinear(_HipModule):
    """deepencoder/build_linear.py:18-19,156 `MlpProjector(projector_type="linear")`: one nn.Linear named `layers`."""

    def __init__(self, input_dim: int, n_embed: int):
        super().__init__()
        self.layers = nn.Linear(input_dim, n_embed)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._autograd(x):
            return self.layers(x)
        self._guard(x)
        shp = x.shape
        y, _ = ops.linear(ops.cast(_f32(x).view(-1, shp[-1]), self._split()), self._w(self.layers.weight), self.layers.bias,
                          out_f32=True)
        return y.view(*shp[:-1], -1)


def deepencoder_fuse(projector: MlpProjectorLinear, clip_tokens: torch.Tensor, sam_feat: torch.Tensor) -> torch.Tensor:
    """deepencoder_infer.py:505-511: cat(clip[:,1:], sam.flatten(2).permute(0,2,1)) -> projector."""
    sam = sam_feat.flatten(2).permute(0, 2, 1)
    return projector(torch.cat((clip_tokens[:, 1:], sam), dim=-1).contiguous())
