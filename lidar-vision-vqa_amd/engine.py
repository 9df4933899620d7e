"""Inference engine on the HIP modules.

Caller contract kept from the reference's `InferenceEngine` (encoder-decoder/inference/inference_engine.py:12-336): the
constructor takes the `models` dict of `ModelLoader.load_all()`; `format_prompt`, `process_lidar`, `process_vision`,
`build_inputs_embeds`, `generate`, `generate_batch` keep their names, arguments and results -- the prompt strings, the marker
tokens and the embedding layout are the interface a checkpoint was trained against, and they are pinned by goldens taken from
the unmodified reference class (tools/make_engine_golden.py).  Everything behind that contract is organised for this build:

  * decoding settings travel as one `Decoding` value; `base_model.generate` may be `StandInHead.generate` (greedy or sampled:
    the reference's DEFAULT call is do_sample=True, temperature 0.7, top_k 50, top_p 0.9 -> lvq_sample_rows) or any
    transformers-style model object;
  * the modal splice is a generic "replace marker pairs" pass over the prompt ids (`_splice`);
  * a stored BEV (fp16 `.npy`, the reference's on-disk format) crosses PCIe as fp16 and is up-cast on the device (`bev.f16_to_f32`).

Two deliberate differences from the reference:
  * it decodes `outputs[0][inputs_embeds.shape[1]:]`, but an inputs_embeds-only `generate` returns ONLY the new tokens, so that
    slice is empty whenever max_new_tokens < prompt length and the reference answers "" (recorded in tests/golden/engine.npz).
    The new tokens are what is decoded here.
  * `process_vision` takes the six per-view token tensors from `models["multiview_tokens_fn"](sample_token)` when that is given;
    otherwise `models["runtime"]` (deepencoder.DeepEncoderRuntime) encodes the six camera files named by
    `models["view_paths_fn"](sample_token)`, or by `resolve_cam_image_paths(nusc, sample_token)`.  Weights are never fetched by URL.
"""
from __future__ import annotations

import inspect
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _ffi as F
from . import bev as B

BevInput = Union[torch.Tensor, np.ndarray, str, Path]
MODALITIES = ("vision", "lidar")            # splice order = the order the markers appear in format_prompt's output


@dataclass(frozen=True)
class Decoding:
    """Settings of one `generate` call, with the reference's defaults (inference_engine.py:236-240)."""
    max_new_tokens: int = 64
    temperature: float = 0.7
    top_p: float = 0.9
    top_k: int = 50
    do_sample: bool = True
    num_beams: int = 1

    def kwargs(self, tokenizer) -> dict:
        """Keyword block for `base_model.generate`; a greedy call carries the neutral warper values, as the reference sends them."""
        warp = dict(temperature=self.temperature, top_p=self.top_p, top_k=self.top_k) if self.do_sample else \
            dict(temperature=1.0, top_p=1.0, top_k=50)
        return dict(max_new_tokens=self.max_new_tokens, do_sample=self.do_sample, num_beams=self.num_beams,
                    pad_token_id=tokenizer.pad_token_id, eos_token_id=tokenizer.eos_token_id, **warp)


def _splice(ids: torch.Tensor, text: torch.Tensor, inserts: Sequence[Tuple[int, int, torch.Tensor]]) -> torch.Tensor:
    """ids [n], text [1, n, d].  For every (start_id, end_id, rows [1, m, d]) in order: the first start marker and the first end
    marker in `ids` stay, `rows` go between them, whatever text sat between them is dropped; a pair with a missing marker is
    skipped.  Text outside the pairs is kept.  Row gathers and one concatenation -- no arithmetic."""
    out, cursor = [], 0
    for start_id, end_id, rows in inserts:
        s = torch.nonzero(ids == start_id).flatten()
        e = torch.nonzero(ids == end_id).flatten()
        if s.numel() == 0 or e.numel() == 0:
            continue
        s0, e0 = int(s[0]), int(e[0])
        out += [text[:, cursor:s0 + 1], rows, text[:, e0:e0 + 1]]
        cursor = e0 + 1
    out.append(text[:, cursor:])
    return torch.cat([t for t in out if t.shape[1] > 0], dim=1)


class Scene:
    """One scene whose modal prefix -- everything `format_prompt` puts in front of the text, up to and including `<lidar_end>` -- has gone
    through the encoders and the head's prefill once (`InferenceEngine.open_scene`).  `ask` answers questions about it from that cache."""

    def __init__(self, engine: "InferenceEngine", lidar: torch.Tensor, vision: Optional[torch.Tensor], rows: torch.Tensor, prefix):
        self.engine, self.lidar, self.vision, self.rows, self.prefix = engine, lidar, vision, rows, prefix

    @property
    def n_rows(self) -> int:
        """P: embedding rows of the cached prefix"""
        return self.rows.shape[1]

    def question_rows(self, question: str) -> torch.Tensor:
        """The embedding rows [1, n, d] of this question's prompt BEHIND the scene's prefix.  The whole prompt is built as `answer` builds
        it and its first P rows must be the scene's, bit for bit (the end marker is a special token, so P is a token boundary)."""
        eng = self.engine
        emb = eng.build_inputs_embeds(eng.format_prompt(question, include_vision=self.vision is not None), self.lidar, self.vision)[0]
        P = self.n_rows
        if emb.shape[1] <= P or not torch.equal(emb[:, :P], self.rows):
            raise F.LvqError("Scene.ask: the prompt of this question does not start with the scene's cached prefix rows")
        return emb[:, P:]

    def ask(self, questions: Sequence[str], **generation_kwargs) -> List[str]:
        """One answer per question, in order, from ONE ragged decode loop behind the cached prefix (`generation_kwargs` as `generate`)."""
        return self.engine._ask_scenes([(self, q) for q in questions], generation_kwargs)


class InferenceEngine:
    def __init__(self, models: Dict):
        need = ("tokenizer", "base_model", "vat_lidar", "config", "device", "d_model")
        missing = [k for k in need if k not in models]
        if missing:
            raise KeyError(f"InferenceEngine: models dict lacks {missing}")
        self.tokenizer, self.base_model, self.vat_lidar = models["tokenizer"], models["base_model"], models["vat_lidar"]
        self.vat_vision, self.vision_adapter = models.get("vat_vision"), models.get("vision_adapter")
        self.runtime, self.nusc = models.get("runtime"), models.get("nusc")
        self.multiview_tokens_fn, self.view_paths_fn = models.get("multiview_tokens_fn"), models.get("view_paths_fn")
        self.config, self.device, self.d_model = models["config"], models["device"], models["d_model"]
        self.use_vision = bool(self.config.get("use_vision", False)) and self.vat_vision is not None
        self.prefix_scale = self.config.get("prefix_scale", 0.2)
        self.system_prompt = self.config.get("system_prompt", "")
        tid = self.tokenizer.convert_tokens_to_ids
        self.marker_ids = {m: (tid(f"<{m}_start>"), tid(f"<{m}_end>")) for m in MODALITIES}
        (self.vision_start_id, self.vision_end_id), (self.lidar_start_id, self.lidar_end_id) = (self.marker_ids[m] for m in MODALITIES)

    # ---- prompt text (the strings a checkpoint is trained against: inference_engine.py:48-70) ----
    def format_prompt(self, question: str, include_vision: bool = True) -> str:
        body = f"{self.system_prompt}\n\n{question}" if self.system_prompt else question
        mods = MODALITIES if (self.use_vision and include_vision) else MODALITIES[1:]
        return "".join(f"<{m}_start><{m}_end>" for m in mods) + f"{body}\nAnswer:"

    # ---- modal prefixes ----
    @torch.no_grad()
    def process_lidar(self, bev: torch.Tensor) -> torch.Tensor:
        """bev [B, C, H, W] or [C, H, W] -> LiDAR prompts [B, n_queries, d_model] (inference_engine.py:72-102)."""
        return self.vat_lidar((bev if bev.ndim == 4 else bev[None]).to(self.device))

    @torch.no_grad()
    def process_vision(self, sample_token: str) -> Optional[torch.Tensor]:
        """Six camera views -> VisionAdapter -> VATVision prompts [1, n_queries, d_model]; None when vision is off
        (inference_engine.py:104-137)."""
        if not self.use_vision:
            return None
        if self.multiview_tokens_fn is None and self.runtime is not None:
            from .deepencoder import resolve_cam_image_paths
            paths = self.view_paths_fn(sample_token) if self.view_paths_fn is not None else resolve_cam_image_paths(self.nusc, sample_token)
            views = [t.to(self.device) for t in self.runtime.encode_views(paths, strict=False)["tokens"]]
            return self.vat_vision(self.vision_adapter(views)[None])
        if self.multiview_tokens_fn is None:
            raise F.LvqError("process_vision: pass models['multiview_tokens_fn'](sample_token) -> six [HW, d_in] tensors; the "
                             "DeepEncoder towers are outside this build (DESIGN section 6)")
        views = [t.to(self.device) for t in self.multiview_tokens_fn(sample_token)]
        return self.vat_vision(self.vision_adapter(views)[None])

    def _load_bev(self, bev: BevInput) -> torch.Tensor:
        if isinstance(bev, (str, Path)):
            bev = np.load(bev)
        if isinstance(bev, np.ndarray):
            if bev.dtype == np.float16:
                return B.f16_to_f32(torch.from_numpy(np.ascontiguousarray(bev)).to(self.device))
            return torch.from_numpy(bev).float()
        return bev

    # ---- prompt embeddings with the scaled prefixes between their markers (inference_engine.py:139-227) ----
    @torch.no_grad()
    def build_inputs_embeds(self, prompt: str, lidar_prompts: torch.Tensor, vision_prompts: Optional[torch.Tensor] = None) -> tuple:
        """Returns (inputs_embeds [1, L, d], all-ones attention mask [1, L])."""
        ids = self.tokenizer(prompt, return_tensors="pt", add_special_tokens=False)["input_ids"].to(self.device)
        text = self.base_model.get_input_embeddings()(ids)
        given = {"vision": vision_prompts if self.use_vision else None, "lidar": lidar_prompts}
        inserts = [(*self.marker_ids[m], given[m] * self.prefix_scale) for m in MODALITIES if given[m] is not None]
        emb = _splice(ids[0], text, inserts)
        return emb, torch.ones(emb.shape[:2], dtype=torch.long, device=self.device)

    # ---- answers ----
    def _prefixes(self, bev: BevInput, sample_token: Optional[str]) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        lidar = self.process_lidar(self._load_bev(bev))
        vision = None
        if self.use_vision and sample_token is not None:
            try:
                vision = self.process_vision(sample_token)
            except Exception as err:       # LiDAR-only answer instead of no answer, like the reference (inference_engine.py:262-268)
                print(f"[engine] vision prefix unavailable for {sample_token!r} ({err}); answering from LiDAR only")
        return lidar, vision

    @torch.no_grad()
    def answer(self, question: str, bev: BevInput, sample_token: Optional[str], decoding: Decoding, generator=None) -> str:
        lidar, vision = self._prefixes(bev, sample_token)
        prompt = self.format_prompt(question, include_vision=vision is not None)
        emb, mask = self.build_inputs_embeds(prompt, lidar, vision)
        extra = {"generator": generator} if generator is not None else {}
        new_ids = self.base_model.generate(inputs_embeds=emb, attention_mask=mask, **decoding.kwargs(self.tokenizer), **extra)
        return self.tokenizer.decode(new_ids[0].tolist(), skip_special_tokens=True).strip()

    def generate(self, question: str, bev: BevInput, sample_token: Optional[str] = None, max_new_tokens: int = 64,
                 temperature: float = 0.7, top_p: float = 0.9, top_k: int = 50, do_sample: bool = True, num_beams: int = 1,
                 generator: Optional[torch.Generator] = None) -> str:
        """The reference's signature and defaults (inference_engine.py:229-240); `generator` seeds the sampled path."""
        return self.answer(question, bev, sample_token, Decoding(max_new_tokens, temperature, top_p, top_k, do_sample, num_beams), generator)

    @torch.no_grad()
    def answer_batch(self, questions: Sequence[str], bevs: Sequence[BevInput], sample_tokens: Optional[Sequence[Optional[str]]],
                     decoding: Decoding, generator=None) -> List[str]:
        """`answer` for several (question, bev[, sample_token]) triples with ONE `base_model.generate` call: the LiDAR prefix runs once on
        the stacked BEVs (once per shape group when the canvases differ), the vision prefix per sample, every prompt is embedded with
        `build_inputs_embeds`, the prompts are right-padded to a common length and decoded as a ragged batch
        (`generate(..., prompt_lengths=)`: head.StandInHead).  A `base_model.generate` without a `prompt_lengths` parameter (a
        transformers model object) gets the per-question loop."""
        n = len(questions)
        tokens = list(sample_tokens) if sample_tokens is not None else [None] * n
        if n == 0:
            return []
        if "prompt_lengths" not in inspect.signature(self.base_model.generate).parameters:
            return [self.answer(q, b, t, decoding, generator) for q, b, t in zip(questions, bevs, tokens)]
        loaded = [self._load_bev(b) for b in bevs]
        loaded = [(b if b.ndim == 4 else b[None]).to(self.device) for b in loaded]
        lidar: List[Optional[torch.Tensor]] = [None] * n
        groups: Dict[tuple, List[int]] = {}
        for i, b in enumerate(loaded):
            if b.shape[0] != 1:
                raise F.LvqError("answer_batch: one BEV canvas ([C, H, W] or [1, C, H, W]) per question")
            groups.setdefault(tuple(b.shape), []).append(i)
        for idx in groups.values():
            rows = self.process_lidar(torch.cat([loaded[i] for i in idx], dim=0))
            for k, i in enumerate(idx):
                lidar[i] = rows[k:k + 1]
        embs = []
        for i, (q, t) in enumerate(zip(questions, tokens)):
            vision = None
            if self.use_vision and t is not None:
                try:
                    vision = self.process_vision(t)
                except Exception as err:       # LiDAR-only answer instead of no answer, as in `_prefixes`
                    print(f"[engine] vision prefix unavailable for {t!r} ({err}); answering from LiDAR only")
            prompt = self.format_prompt(q, include_vision=vision is not None)
            embs.append(self.build_inputs_embeds(prompt, lidar[i], vision)[0])
        lens = torch.tensor([e.shape[1] for e in embs], dtype=torch.int32, device=self.device)
        width = max(e.shape[1] for e in embs)
        batch = torch.zeros((n, width, embs[0].shape[2]), dtype=embs[0].dtype, device=self.device)
        for i, e in enumerate(embs):
            batch[i, :e.shape[1]] = e[0]
        mask = (torch.arange(width, device=self.device)[None, :] < lens[:, None]).long()
        extra = {"generator": generator} if generator is not None else {}
        new_ids = self.base_model.generate(inputs_embeds=batch, attention_mask=mask, prompt_lengths=lens, **decoding.kwargs(self.tokenizer), **extra)
        return self._decode_rows(new_ids)

    def _decode_rows(self, new_ids: torch.Tensor) -> List[str]:
        eos = self.tokenizer.eos_token_id
        out = []
        for row in new_ids.tolist():
            if eos is not None and eos in row:             # what the sequence's own loop returns: it stops with its EOS
                row = row[:row.index(eos) + 1]
            out.append(self.tokenizer.decode(row, skip_special_tokens=True).strip())
        return out

    # ---- many questions about one scene: the modal prefix is encoded and prefilled once ----
    @torch.no_grad()
    def open_scene(self, bev: BevInput, sample_token: Optional[str] = None) -> Scene:
        """`process_lidar` (and `process_vision`) once, then the head's prefill of the prompt rows up to and including `<lidar_end>`
        (`base_model.prefill_prefix`: head.StandInHead).  The result answers any number of questions with `Scene.ask`."""
        if not callable(getattr(self.base_model, "prefill_prefix", None)):
            raise F.LvqError("open_scene: base_model has no prefill_prefix (head.StandInHead has); use generate / generate_batch")
        lidar, vision = self._prefixes(bev, sample_token)
        if lidar.shape[0] != 1:
            raise F.LvqError("open_scene: one BEV canvas ([C, H, W] or [1, C, H, W]) per scene")
        # format_prompt puts the modal blocks first; the rows behind <lidar_end> of this question-less prompt are dropped
        prompt = self.format_prompt("", include_vision=vision is not None)
        ids = self.tokenizer(prompt, return_tensors="pt", add_special_tokens=False)["input_ids"][0]
        end = torch.nonzero(ids == self.lidar_end_id).flatten()
        if end.numel() == 0:
            raise F.LvqError("open_scene: the prompt carries no <lidar_end> marker")
        n_tail = ids.numel() - 1 - int(end[0])                 # text tokens behind the marker
        emb = self.build_inputs_embeds(prompt, lidar, vision)[0]
        rows = emb[:, :emb.shape[1] - n_tail].contiguous()
        return Scene(self, lidar, vision, rows, self.base_model.prefill_prefix(rows))

    @torch.no_grad()
    def _ask_scenes(self, pairs: Sequence[Tuple[Scene, str]], generation_kwargs: dict) -> List[str]:
        """[(scene, question)] -> answers in order, with ONE `base_model.generate` call.  The scenes' caches must be one PrefixCache or
        single-prefix caches of equal width; several of them are stacked (byte movement) so that `prefix_index` selects among them."""
        if not pairs:
            return []
        kw = dict(generation_kwargs)
        generator = kw.pop("generator", None)
        decoding = Decoding(**kw)
        scenes: List[Scene] = []
        for sc, _ in pairs:
            if not any(sc is s for s in scenes):
                scenes.append(sc)
        prefix = scenes[0].prefix if len(scenes) == 1 else self._stack_prefixes([s.prefix for s in scenes])
        index = [next(i for i, s in enumerate(scenes) if s is sc) for sc, _ in pairs]
        embs = [sc.question_rows(q) for sc, q in pairs]
        n = len(embs)
        lens = torch.tensor([e.shape[1] for e in embs], dtype=torch.int32, device=self.device)
        width = max(e.shape[1] for e in embs)
        batch = torch.zeros((n, width, embs[0].shape[2]), dtype=embs[0].dtype, device=self.device)
        for i, e in enumerate(embs):
            batch[i, :e.shape[1]] = e[0]
        mask = (torch.arange(width, device=self.device)[None, :] < lens[:, None]).long()
        extra = {"generator": generator} if generator is not None else {}
        new_ids = self.base_model.generate(inputs_embeds=batch, attention_mask=mask, prompt_lengths=lens, prefix=prefix,
                                           prefix_index=torch.tensor(index, dtype=torch.int32, device=self.device),
                                           **decoding.kwargs(self.tokenizer), **extra)
        return self._decode_rows(new_ids)

    @staticmethod
    def _stack_prefixes(prefixes):
        """Single-scene PrefixCaches -> one cache [G, pmax, dkv] per layer for a call that mixes scenes (row copies; no arithmetic)."""
        from .head import PrefixCache
        first = prefixes[0]
        pmax = max(p.pmax for p in prefixes)
        if any(p.mode != first.mode or p.version != first.version or p.owner() is not first.owner() for p in prefixes):
            raise F.LvqError("scenes of one call must come from the same head, weights and precision mode")

        def stack(parts):
            if parts[0] is None:
                return None
            out = torch.zeros((sum(t.shape[0] for t in parts), pmax, parts[0].shape[2]), dtype=parts[0].dtype, device=parts[0].device)
            g = 0
            for t in parts:
                out[g:g + t.shape[0], :t.shape[1]] = t
                g += t.shape[0]
            return out
        layers = []
        for i in range(len(first.layers)):
            layers.append(tuple(tuple(stack([p.layers[i][kv][part] for p in prefixes]) for part in (0, 1)) for kv in (0, 1)))
        return PrefixCache(layers, torch.cat([p.plen for p in prefixes]), [n for p in prefixes for n in p.lengths], pmax, first.mode,
                           first.version, first.owner)

    def generate_batch(self, questions: List[str], bevs: List[BevInput], sample_tokens: Optional[List[str]] = None, batch_size: int = 1,
                       share_scenes: bool = False, **generation_kwargs) -> List[str]:
        """One answer per (question, bev[, sample_token]) triple, in order (inference_engine.py:306-336).  The questions are answered in
        groups of `batch_size`: a group of one is a `generate` call (the default: the reference's loop), a larger group is one
        `answer_batch` call -- one LiDAR pass and one ragged decode loop for the group.  `batch_size` is the caller's memory / latency
        choice; greedy answers do not depend on it beyond the precision mode's rounding.

        share_scenes=True: triples with the same `sample_token` and the same BEV (the same path string or the same object; contents are
        not hashed) are questions about ONE scene.  Every scene is opened once (`open_scene`: one LiDAR pass, one prefill of its modal
        prefix) when its first question comes up and released behind its last one, and groups of `batch_size` questions -- of one scene or of several -- decode in one loop behind the cached prefixes
        (`generate(prefix=, prefix_index=)`).  Answers come back in input order.  A `base_model` whose `generate` has no `prefix`
        parameter gets the path above."""
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        tokens = sample_tokens if sample_tokens is not None else [None] * len(questions)
        triples = list(zip(questions, bevs, tokens))
        if share_scenes and "prefix" in inspect.signature(self.base_model.generate).parameters:
            # a scene is opened when its first question comes up and dropped behind its last one: a QA file with thousands of sample
            # tokens holds the prefix caches of the scenes of ONE group at a time (plus those that straddle a group boundary)
            keys = [(t, str(b) if isinstance(b, (str, Path)) else id(b)) for _, b, t in triples]
            last = {k: i for i, k in enumerate(keys)}
            scenes: Dict[tuple, Scene] = {}
            shared: List[str] = []
            for i in range(0, len(triples), batch_size):
                pairs = []
                for (q, b, t), k in zip(triples[i:i + batch_size], keys[i:i + batch_size]):
                    if k not in scenes:
                        scenes[k] = self.open_scene(b, t)
                    pairs.append((scenes[k], q))
                shared += self._ask_scenes(pairs, generation_kwargs)
                for k in [k for k in scenes if last[k] < i + batch_size]:
                    del scenes[k]
            return shared
        out: List[str] = []
        for i in range(0, len(triples), batch_size):
            group = triples[i:i + batch_size]
            if len(group) == 1:
                out.append(self.generate(*group[0], **generation_kwargs))
            else:
                kw = dict(generation_kwargs)
                generator = kw.pop("generator", None)
                qs, bs, ts = zip(*group)
                out += self.answer_batch(qs, bs, ts, Decoding(**kw), generator)
        return out
