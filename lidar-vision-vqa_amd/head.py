"""Prefix assembly + stand-in language head.

The reference concatenates `[E(<vision_start>), prefix_vision*s, E(<vision_end>), E(<lidar_start>),
prefix_lidar*s, E(<lidar_end>), E(prompt), E(answer)]` and calls
`base(inputs_embeds=..., attention_mask=ones, labels=...)` on a LoRA-wrapped `Qwen/Qwen2.5-0.5B`
(encoder-decoder/training/core/validation.py:105-158, trainer.py:568-675,
inference/inference_engine.py:139-227).  That checkpoint is fetched by name -> unreachable offline, so the
head here is a random-init decoder of the SAME architecture (transformers' Qwen2ForCausalLM: RMSNorm,
rotary GQA self-attention with q/k/v bias, SwiGLU, tied lm_head, shifted cross-entropy) with the SAME
state_dict keys, pinned against transformers in tests/golden/head_prefix.npz.  LoRA-B is zero at init,
so a LoRA-wrapped base equals the base for an untrained-weights parity test.
"""
from __future__ import annotations

import math
import os
import weakref
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import _ffi as F
from . import ops
from .fusion import _HipModule, _f32


def assemble_prefix(prefix_vision: Optional[torch.Tensor], prefix_lidar: Optional[torch.Tensor], e_special: torch.Tensor,
                    e_prompt: torch.Tensor, e_answer: torch.Tensor, answer_ids: torch.Tensor, prefix_scale: float = 0.2
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Eval order VISION -> LIDAR -> TEXT -> ANSWER, prompt appended once (validation.py:125-148).
    e_special rows: <vision_start>, <vision_end>, <lidar_start>, <lidar_end>.
    Returns inputs_embeds [B,L,d], attention_mask [B,L] (ones), labels [B,L] (-100 except the answer span)."""
    B = e_prompt.shape[0]
    pieces = []

    def scaled(p):
        return ops.scale_add_rows(_f32(p).view(-1, p.shape[-1]), None, prefix_scale).view_as(p)
    if prefix_vision is not None:
        pieces += [e_special[0].expand(B, 1, -1), scaled(prefix_vision), e_special[1].expand(B, 1, -1)]
    if prefix_lidar is not None:
        pieces += [e_special[2].expand(B, 1, -1), scaled(prefix_lidar), e_special[3].expand(B, 1, -1)]
    pieces.append(e_prompt)
    inp = torch.cat(pieces + [e_answer], dim=1).contiguous()
    L = inp.shape[1]
    labels = torch.full((B, L), -100, dtype=torch.long, device=inp.device)
    labels[:, -answer_ids.shape[1]:] = answer_ids
    attn = torch.ones((B, L), dtype=torch.long, device=inp.device)
    return inp, attn, labels


class _Weight(nn.Module):
    """RMSNorm parameter container (key `<name>.weight`)."""

    def __init__(self, d):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))


class _Attn(nn.Module):
    def __init__(self, d, dkv):
        super().__init__()
        self.q_proj = nn.Linear(d, d, bias=True)
        self.k_proj = nn.Linear(d, dkv, bias=True)
        self.v_proj = nn.Linear(d, dkv, bias=True)
        self.o_proj = nn.Linear(d, d, bias=False)


class _Mlp(nn.Module):
    def __init__(self, d, inter):
        super().__init__()
        self.gate_proj = nn.Linear(d, inter, bias=False)
        self.up_proj = nn.Linear(d, inter, bias=False)
        self.down_proj = nn.Linear(inter, d, bias=False)


class _Layer(nn.Module):
    def __init__(self, d, dkv, inter):
        super().__init__()
        self.self_attn = _Attn(d, dkv)
        self.mlp = _Mlp(d, inter)
        self.input_layernorm = _Weight(d)
        self.post_attention_layernorm = _Weight(d)


class _Model(nn.Module):
    def __init__(self, vocab, d, dkv, inter, n_layers):
        super().__init__()
        self.embed_tokens = nn.Embedding(vocab, d)
        self.layers = nn.ModuleList([_Layer(d, dkv, inter) for _ in range(n_layers)])
        self.norm = _Weight(d)


import ctypes as _ct


class _Qwen2LayerPtrs(_ct.Structure):
    """include/lvq.h: lvq_qwen2_layer (device pointers of one decoder layer)."""
    _fields_ = [(n, _ct.c_void_p) for n in ("ln1", "ln2", "wqkv", "wqkv_lo", "bqkv", "wo", "wo_lo", "wgu", "wgu_lo", "wdown", "wdown_lo",
                                             "k_cache", "k_cache_lo", "v_cache", "v_cache_lo")]


class _Qwen2PrefixPtrs(_ct.Structure):
    """include/lvq.h: lvq_qwen2_prefix (device pointers of one layer's shared prefix caches)."""
    _fields_ = [(n, _ct.c_void_p) for n in ("k", "k_lo", "v", "v_lo")]


class PrefixCache:
    """What `StandInHead.prefill_prefix` keeps of G prefixes for `generate(prefix=)`: per layer the K / V rows [G, pmax, dkv] (hi, and lo in
    the bf16x3 mode), the lengths `plen` (int32 [G] on the device; `lengths` the same numbers on the host), and what the rows were
    computed with -- the head, its precision mode and the version of its weights.  Read-only: any number of generate calls may use it."""

    def __init__(self, layers, plen, lengths, pmax, mode, version, owner):
        self.layers, self.plen, self.lengths, self.pmax, self.mode, self.version, self.owner = layers, plen, lengths, pmax, mode, version, owner

    @property
    def n_prefix(self) -> int:
        return len(self.lengths)


class HeadOutput:
    def __init__(self, logits, loss):
        self.logits, self.loss = logits, loss


class StandInHead(_HipModule):
    """Qwen2-architecture causal LM; call like the reference's `base(inputs_embeds=, attention_mask=, labels=)`."""

    def __init__(self, vocab: int, d: int, inter: int, n_heads: int, n_kv_heads: int, n_layers: int, rms_eps: float = 1e-6,
                 rope_theta: float = 1000000.0):
        super().__init__()
        assert d % n_heads == 0 and n_heads % n_kv_heads == 0
        self.dh = d // n_heads
        assert self.dh % 16 == 0 and self.dh <= 128, "stand-in head uses the fused attention kernel (head_dim multiple of 16, <= 128)"
        self.cfg = dict(vocab=vocab, d=d, inter=inter, n_heads=n_heads, n_kv_heads=n_kv_heads, n_layers=n_layers, rms_eps=rms_eps,
                        rope_theta=rope_theta)
        dkv = self.dh * n_kv_heads
        self.model = _Model(vocab, d, dkv, inter, n_layers)
        self.lm_head = nn.Linear(d, vocab, bias=False)
        self.lm_head.weight = self.model.embed_tokens.weight      # tie_word_embeddings=True
        object.__setattr__(self, "_packed", {})

    def get_input_embeddings(self):
        return self.model.embed_tokens

    def embed(self, ids: torch.Tensor) -> torch.Tensor:
        """E(ids): a row gather of the embedding table (byte movement)."""
        return self.model.embed_tokens.weight.detach()[ids]

    def _pack(self, key, params, biases=None):
        """Concatenated projection weights (q|k|v, gate|up) as one GEMM operand; rebuilt when a member changes."""
        split = self._split()

        def build():
            w = ops.cast(torch.cat([p.detach().float() for p in params], dim=0).contiguous(), split)
            return w, (torch.cat([p.detach().float() for p in biases]).contiguous() if biases else None)
        return F.derived(self._packed, key, params, build, (split,))

    def _layers(self, x: torch.Tensor, B: int, Lq: int, pos0: int = 0, cache=None) -> torch.Tensor:
        """The decoder stack on rows x [B*Lq, d] = positions pos0 .. pos0+Lq-1 of every sequence.  cache = None: plain causal
        self-attention over these rows (training-eval path).  cache = list of per-layer ((k_hi, k_lo), (v_hi, v_lo)) buffers
        [B, Lmax, dkv]: the new keys / values are appended at pos0 and attention runs over positions 0 .. pos0+Lq-1."""
        c = self.cfg
        d = c["d"]
        H, Hk, dh = c["n_heads"], c["n_kv_heads"], self.dh
        dkv = dh * Hk
        split = self._split()
        ld = d + 2 * dkv
        sl = lambda t, c0: (t[0][:, c0:], None if t[1] is None else t[1][:, c0:])
        for i, layer in enumerate(self.model.layers):
            a = layer.self_attn
            h = ops.rmsnorm(x, layer.input_layernorm.weight, c["rms_eps"], split)
            wqkv, bqkv = self._pack(("qkv", i), (a.q_proj.weight, a.k_proj.weight, a.v_proj.weight),
                                    (a.q_proj.bias, a.k_proj.bias, a.v_proj.bias))
            _, qkv = ops.linear(h, wqkv, bqkv, out_bf=True)
            ops.rope_inplace(sl(qkv, 0), B * Lq, Lq, H, dh, ld, c["rope_theta"], pos0)
            ops.rope_inplace(sl(qkv, d), B * Lq, Lq, Hk, dh, ld, c["rope_theta"], pos0)
            st = (Lq * ld, ld, dh)
            if cache is None:
                o = ops.attention(sl(qkv, 0), sl(qkv, d), sl(qkv, d + dkv), batch=B, n_heads=H, n_kv_heads=Hk, nq=Lq, nkv=Lq, dh=dh,
                                  q_strides=st, k_strides=st, v_strides=st, scale=1.0 / math.sqrt(dh), causal=True)
            else:
                kc, vc = cache[i]
                lmax = kc[0].shape[1]
                for part in (0, 1):                       # hi (and lo in the bf16x3 mode): byte movement into the cache
                    if qkv[part] is None:
                        continue
                    rows = qkv[part].view(B, Lq, ld)
                    kc[part][:, pos0:pos0 + Lq].copy_(rows[:, :, d:d + dkv])
                    vc[part][:, pos0:pos0 + Lq].copy_(rows[:, :, d + dkv:])
                cs = (lmax * dkv, dkv, dh)
                o = ops.attention(sl(qkv, 0), kc, vc, batch=B, n_heads=H, n_kv_heads=Hk, nq=Lq, nkv=pos0 + Lq, dh=dh,
                                  q_strides=st, k_strides=cs, v_strides=cs, scale=1.0 / math.sqrt(dh), causal=Lq > 1)
            x, _ = ops.linear(o, self._w(a.o_proj.weight), None, residual=x, out_f32=True)
            h = ops.rmsnorm(x, layer.post_attention_layernorm.weight, c["rms_eps"], split)
            wgu, _ = self._pack(("gu", i), (layer.mlp.gate_proj.weight, layer.mlp.up_proj.weight))
            gu, _ = ops.linear(h, wgu, None, out_f32=True)
            act = ops.swiglu(gu, split)
            x, _ = ops.linear(act, self._w(layer.mlp.down_proj.weight), None, residual=x, out_f32=True)
        return x

    def _logits(self, x: torch.Tensor) -> torch.Tensor:
        hf = ops.rmsnorm(x, self.model.norm.weight, self.cfg["rms_eps"], self._split())
        logits, _ = ops.linear(hf, self._w(self.model.embed_tokens.weight), None, out_f32=True)
        return logits

    def forward(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                labels: Optional[torch.Tensor] = None) -> HeadOutput:
        self._guard(inputs_embeds)
        B, L, d = inputs_embeds.shape
        x = self._layers(_f32(inputs_embeds).view(B * L, d), B, L)
        logits = self._logits(x)
        loss = None
        if labels is not None:
            shifted = torch.full_like(labels, -100)
            shifted[:, :-1] = labels[:, 1:]
            loss = ops.cross_entropy(logits, shifted.reshape(-1).contiguous())
        return HeadOutput(logits.view(B, L, -1), loss)

    def _native_layers(self, cache):
        """Host array of lvq_qwen2_layer structs for lvq_qwen2_decode_step + the tensors that must stay alive behind it."""
        keep, arr = [], (_Qwen2LayerPtrs * len(self.model.layers))()
        p = lambda t: None if t is None else t.data_ptr()
        for i, layer in enumerate(self.model.layers):
            a = layer.self_attn
            wqkv, bqkv = self._pack(("qkv", i), (a.q_proj.weight, a.k_proj.weight, a.v_proj.weight),
                                    (a.q_proj.bias, a.k_proj.bias, a.v_proj.bias))
            wo = self._w(a.o_proj.weight)
            wgu, _ = self._pack(("gu", i), (layer.mlp.gate_proj.weight, layer.mlp.up_proj.weight))
            wd = self._w(layer.mlp.down_proj.weight)
            ln1 = layer.input_layernorm.weight.detach().float().contiguous()
            ln2 = layer.post_attention_layernorm.weight.detach().float().contiguous()
            (kh, kl), (vh, vl) = cache[i]
            keep += [wqkv, bqkv, wo, wgu, wd, ln1, ln2]
            arr[i] = _Qwen2LayerPtrs(p(ln1), p(ln2), p(wqkv[0]), p(wqkv[1]), p(bqkv), p(wo[0]), p(wo[1]), p(wgu[0]), p(wgu[1]),
                                     p(wd[0]), p(wd[1]), p(kh), p(kl), p(vh), p(vl))
        return arr, keep

    def _ragged_prompts(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor], prompt_lengths: torch.Tensor):
        """Checks of a ragged generate call.  Returns (inputs_embeds with the padding rows zeroed, prompt lengths as int32 [B] on the
        device = pos0 of lvq_qwen2_decode_step_ragged)."""
        B, L, _ = inputs_embeds.shape
        dev = inputs_embeds.device
        if not isinstance(prompt_lengths, torch.Tensor) or prompt_lengths.is_floating_point() or prompt_lengths.dtype == torch.bool \
                or tuple(prompt_lengths.shape) != (B,):
            raise F.LvqError(f"StandInHead.generate: prompt_lengths must be an integer tensor of shape [{B}]")
        lens = prompt_lengths.to(device=dev, dtype=torch.long)
        if not bool(((lens >= 1) & (lens <= L)).all()):
            raise F.LvqError(f"StandInHead.generate: prompt_lengths must lie in 1 .. {L}")
        real = torch.arange(L, device=dev)[None, :] < lens[:, None]                     # [B, L]: right-padded layout
        if attention_mask is not None:
            if tuple(attention_mask.shape) != (B, L) or not bool(((attention_mask.to(dev) != 0) == real).all()):
                raise F.LvqError("StandInHead.generate: with prompt_lengths the attention_mask must be None or the right-padded mask of "
                                 "those lengths (left padding is not supported)")
        emb = torch.where(real[:, :, None], inputs_embeds, torch.zeros((), dtype=inputs_embeds.dtype, device=dev))
        return emb, lens.to(torch.int32).contiguous()

    def _weights_version(self):
        return F.version_of(self.parameters())

    @torch.no_grad()
    def prefill_prefix(self, inputs_embeds: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> PrefixCache:
        """The decoder stack on G prompt prefixes [G, P, d] (one causal prefill, the call `generate` makes for a prompt), kept as a
        `PrefixCache` that later `generate(prefix=)` calls continue.  lengths = None: every prefix has P rows; an int tensor [G] with
        1 <= lengths[g] <= P: prefix g is rows 0 .. lengths[g]-1, the rows behind it are padding (zeroed here; causality keeps them out of
        the real rows, and no later call reads their K / V)."""
        self._guard(inputs_embeds)
        G, P, d = inputs_embeds.shape
        dev = inputs_embeds.device
        if lengths is None:
            lengths = torch.full((G,), P, dtype=torch.int32, device=dev)
        emb, plen = self._ragged_prompts(inputs_embeds, None, lengths)
        dkv = self.dh * self.cfg["n_kv_heads"]
        split = self._split()
        mk = lambda: (torch.empty((G, P, dkv), dtype=torch.bfloat16, device=dev),
                      torch.empty((G, P, dkv), dtype=torch.bfloat16, device=dev) if split else None)
        cache = [(mk(), mk()) for _ in self.model.layers]
        self._layers(_f32(emb).view(G * P, d), G, P, 0, cache)
        return PrefixCache(cache, plen, [int(n) for n in plen.tolist()], P, self._mode(), self._weights_version(), weakref.ref(self))

    def _shared_prompts(self, inputs_embeds, attention_mask, prompt_lengths, prefix, prefix_index):
        """Checks of a generate call that continues a PrefixCache.  Returns (rows behind the prefix with the padding zeroed, their counts as
        int32 [B], prefix_index as int32 [B])."""
        B, L, _ = inputs_embeds.shape
        dev = inputs_embeds.device
        if not isinstance(prefix, PrefixCache) or prefix.owner() is not self:
            raise F.LvqError("StandInHead.generate: prefix must be a PrefixCache made by this head's prefill_prefix")
        if prefix.mode != self._mode():
            raise F.LvqError(f"StandInHead.generate: the prefix was computed in precision mode {prefix.mode!r}, the head now runs {self._mode()!r}")
        if prefix.version != self._weights_version():
            raise F.LvqError("StandInHead.generate: the head's weights changed after prefill_prefix; compute the prefix again")
        if prefix.plen.device != dev:
            raise F.LvqError("StandInHead.generate: the prefix lives on another device")
        if prefix_index is None:
            if prefix.n_prefix != 1:
                raise F.LvqError("StandInHead.generate: a PrefixCache of several prefixes needs prefix_index [B]")
            prefix_index = torch.zeros(B, dtype=torch.int32, device=dev)
        if not isinstance(prefix_index, torch.Tensor) or prefix_index.is_floating_point() or prefix_index.dtype == torch.bool \
                or tuple(prefix_index.shape) != (B,):
            raise F.LvqError(f"StandInHead.generate: prefix_index must be an integer tensor of shape [{B}]")
        pidx = prefix_index.to(device=dev, dtype=torch.long)
        if not bool(((pidx >= 0) & (pidx < prefix.n_prefix)).all()):
            raise F.LvqError(f"StandInHead.generate: prefix_index must lie in 0 .. {prefix.n_prefix - 1}")
        if prompt_lengths is None:
            prompt_lengths = torch.full((B,), L, dtype=torch.int32, device=dev)
        emb, qlen = self._ragged_prompts(inputs_embeds, attention_mask, prompt_lengths)
        return emb, qlen, pidx.to(torch.int32).contiguous()

    def _extend_shared(self, layers_arr, prefix_arr, prefix, pidx, rows, B, lq, own0, qn, t, lown, prec, ws):
        """lvq_qwen2_extend_shared on rows [B * lq, d] fp32, in place: sequence b continues prefix pidx[b] behind own0[b] + t own rows."""
        c = self.cfg
        rc = F.lib().lvq_qwen2_extend_shared(layers_arr, prefix_arr, len(self.model.layers), F.ptr(rows), B, lq,
                                             c["d"], c["n_heads"], c["n_kv_heads"], c["inter"], F.ptr(pidx),
                                             F.ptr(prefix.plen), prefix.n_prefix, prefix.pmax, F.ptr(own0), F.ptr(qn), t,
                                             lown, c["rms_eps"], c["rope_theta"], prec, F.ptr(ws),
                                             ws.numel(), F.stream_ptr(rows.device))
        F.check(rc, "lvq_qwen2_extend_shared")

    @torch.no_grad()
    def generate(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, max_new_tokens: int = 64,
                 do_sample: bool = False, num_beams: int = 1, pad_token_id: Optional[int] = None,
                 eos_token_id: Optional[int] = None, output_scores: bool = False, temperature: float = 1.0, top_k: Optional[int] = 50,
                 top_p: float = 1.0, generator: Optional[torch.Generator] = None, prompt_lengths: Optional[torch.Tensor] = None,
                 prefix: Optional[PrefixCache] = None, prefix_index: Optional[torch.Tensor] = None, **unused):
        """`base_model.generate(inputs_embeds=, attention_mask=, max_new_tokens=, temperature=, top_p=, top_k=, do_sample=,
        num_beams=1, pad_token_id=, eos_token_id=)` as inference_engine.py:283-296 calls it, with a per-layer KV cache.
        do_sample=False: greedy (first maximum).  do_sample=True (the reference's default, temperature 0.7 / top_k 50 / top_p 0.9):
        every step draws from transformers' warped distribution (temperature -> top-k -> top-p) with lvq_sample_rows; the uniforms
        come from torch's RNG (`generator` or torch.manual_seed), so runs are reproducible but -- like any two sampling
        implementations -- not stream-identical to transformers' multinomial.  Returns the NEW token ids [B, n] (what transformers
        returns when only inputs_embeds is given); with output_scores=True also the per-step raw logits [B, n, V].  Beam search
        is not built.

        prompt_lengths = None: every row of inputs_embeds is a whole prompt (all-ones attention_mask).  prompt_lengths = int tensor
        [B] with 1 <= prompt_lengths[b] <= L: a RAGGED batch -- row b holds its prompt in positions 0 .. len_b-1, the rows behind it
        are padding (zeroed here; attention_mask is None or the matching right-padded mask).  The prefill is the same causal call
        over L rows (padding lies behind the real rows, so causality keeps it out of them), the first logits come from row len_b-1,
        and every decode step is one lvq_qwen2_decode_step_ragged call with sequence b at position len_b + t, so each sequence sees
        what it would see alone.  Ragged calls exist in the native step only: with LVQ_DECODE_PYTHON set they raise LvqError.

        prefix = a `PrefixCache` of this head's `prefill_prefix`, prefix_index = int tensor [B] (optional for a cache of one prefix):
        sequence b CONTINUES prefix prefix_index[b].  inputs_embeds [B, Lq, d] then holds only the rows behind the prefix and
        prompt_lengths (default: Lq for all) counts those rows.  The prefix rows are neither recomputed nor copied: the question prefill
        is one lvq_qwen2_extend_shared call (csrc/decode_shared.hip) and every decode step is one more with one query row per sequence,
        reading the prefix K / V in place; the sequence's own caches hold Lq + max_new_tokens rows.  A prefix from another head,
        from other weights or from another precision mode raises LvqError, and so does LVQ_DECODE_PYTHON."""
        self._guard(inputs_embeds)
        if num_beams != 1:
            raise F.LvqError("StandInHead.generate: beam search is not implemented (num_beams must be 1)")
        if do_sample and not (temperature > 0.0 and 0.0 < top_p <= 1.0):
            raise ValueError("temperature must be > 0 and top_p in (0, 1]")
        shared = prefix is not None
        if prefix_index is not None and not shared:
            raise F.LvqError("StandInHead.generate: prefix_index without a prefix")
        ragged = prompt_lengths is not None and not shared
        if not ragged and not shared and attention_mask is not None and not bool((attention_mask == 1).all()):
            raise F.LvqError("StandInHead.generate expects an all-ones attention_mask (the reference builds exactly that)")
        c = self.cfg
        B, L, d = inputs_embeds.shape
        dkv = self.dh * c["n_kv_heads"]
        dev = inputs_embeds.device
        if ragged:
            inputs_embeds, pos0 = self._ragged_prompts(inputs_embeds, attention_mask, prompt_lengths)
        elif shared:
            inputs_embeds, qlen, pidx = self._shared_prompts(inputs_embeds, attention_mask, prompt_lengths, prefix, prefix_index)
        lmax = L + max_new_tokens                              # with a prefix: rows of the sequences' OWN caches
        split = self._split()
        mk = lambda: (torch.empty((B, lmax, dkv), dtype=torch.bfloat16, device=dev),
                      torch.empty((B, lmax, dkv), dtype=torch.bfloat16, device=dev) if split else None)
        cache = [(mk(), mk()) for _ in self.model.layers]
        native = not os.environ.get("LVQ_DECODE_PYTHON")       # decode steps: one native call per token (csrc/decoder.hip)
        if shared and not native:
            raise F.LvqError("StandInHead.generate: a call with a prefix has no Python-driven decode loop; unset LVQ_DECODE_PYTHON")
        if not shared:
            x = self._layers(_f32(inputs_embeds).view(B * L, d), B, L, 0, cache)      # prefill
        if ragged and not native:
            raise F.LvqError("StandInHead.generate: a ragged batch (prompt_lengths) has no Python-driven decode loop; unset LVQ_DECODE_PYTHON")
        if shared:
            lib = F.lib()
            layers_arr, keep = self._native_layers(cache)
            prec = 3 if split else 1
            prefix_arr = (_Qwen2PrefixPtrs * len(self.model.layers))()
            for i, ((kh, kl), (vh, vl)) in enumerate(prefix.layers):
                prefix_arr[i] = _Qwen2PrefixPtrs(kh.data_ptr(), None if kl is None else kl.data_ptr(), vh.data_ptr(),
                                                 None if vl is None else vl.data_ptr())
            nbytes = max(int(lib.lvq_qwen2_extend_shared_workspace_bytes(B, lq, d, c["n_heads"],
                                                                         c["n_kv_heads"], c["inter"], prefix.pmax,
                                                                         lmax, prec)) for lq in (L, 1))
            step_ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            zeros, ones = torch.zeros(B, dtype=torch.int32, device=dev), torch.ones(B, dtype=torch.int32, device=dev)
            extend = lambda rows, lq, own0, qn, t: self._extend_shared(layers_arr, prefix_arr, prefix, pidx, rows, B, lq, own0, qn, t, lmax,
                                                                       prec, step_ws)
            x = _f32(inputs_embeds).view(B * L, d)             # _shared_prompts made this copy: the call works in place
            extend(x, L, zeros, qlen, 0)                       # question prefill: own rows 0 .. qlen[b]-1
            pos0 = qlen
        elif native:
            lib = F.lib()
            layers_arr, keep = self._native_layers(cache)
            prec = 3 if split else 1
            ws_query = lib.lvq_qwen2_decode_ragged_workspace_bytes if ragged else lib.lvq_qwen2_decode_workspace_bytes
            nbytes = ws_query(B, d, c["n_heads"], c["n_kv_heads"], c["inter"], lmax, prec)
            step_ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        if ragged or shared:                                   # last real row of every sequence
            last = x.view(B, L, d)[torch.arange(B, device=dev), pos0.long() - 1].contiguous()
        else:
            last = x.view(B, L, d)[:, -1].contiguous()
        step_logits = self._logits(last)                                                # [B, V]
        pad = 0 if pad_token_id is None else int(pad_token_id)
        unfinished = torch.ones(B, dtype=torch.bool, device=dev)
        ids, scores = [], []
        for t in range(max_new_tokens):
            nxt = ops.sample_rows(step_logits, temperature, top_k, top_p, generator) if do_sample else ops.argmax_rows(step_logits)
            if eos_token_id is not None:
                nxt = torch.where(unfinished, nxt, torch.full_like(nxt, pad))
            ids.append(nxt)
            if output_scores:
                scores.append(step_logits)
            if eos_token_id is not None:
                unfinished = unfinished & (nxt != int(eos_token_id))
                if not bool(unfinished.any()):                                          # host sync, as in transformers' loop
                    break
            if t + 1 == max_new_tokens:
                break
            x = self.embed(nxt).float().contiguous()
            if shared:                                         # sequence b: own row qlen[b] + t, one query row (csrc/decode_shared.hip)
                extend(x, 1, qlen, ones, t)
            elif ragged:                                         # sequence b at position pos0[b] + t (csrc/decode_ragged.hip)
                rc = lib.lvq_qwen2_decode_step_ragged(layers_arr, len(self.model.layers), F.ptr(x), B, d,
                                                      c["n_heads"], c["n_kv_heads"], c["inter"], F.ptr(pos0), t,
                                                      lmax, c["rms_eps"], c["rope_theta"], prec,
                                                      F.ptr(step_ws), step_ws.numel(), F.stream_ptr(dev))
                F.check(rc, "lvq_qwen2_decode_step_ragged")
            elif native:
                rc = lib.lvq_qwen2_decode_step(layers_arr, len(self.model.layers), F.ptr(x), B, d,
                                               c["n_heads"], c["n_kv_heads"], c["inter"], L + t, lmax,
                                               c["rms_eps"], c["rope_theta"], prec, F.ptr(step_ws),
                                               step_ws.numel(), F.stream_ptr(dev))
                F.check(rc, "lvq_qwen2_decode_step")
            else:
                x = self._layers(x, B, 1, L + t, cache)
            step_logits = self._logits(x)
        out = torch.stack(ids, dim=1)
        return (out, torch.stack(scores, dim=1)) if output_scores else out
