#!/usr/bin/env python3
"""Many questions about one scene: `generate_batch` per question (batch_size = 1), in ragged groups (batch_size = 8) and from a cached
scene prefix (share_scenes = True; csrc/decode_shared.hip), plus a variant that COPIES the cached prefix rows into per-question caches and
decodes with the ragged step -- the alternative to a kernel that reads the prefix in place.

Geometry: Qwen2.5-0.5B as README quotes it (d 896, 14 / 2 heads, head_dim 64, inter 4864, 24 layers), random weights, vocabulary CUT to
8192 rows.  LiDAR-only prompts: VATLiDAR(64 channels, 32 x 32 canvas, 840 queries, 2 blocks) -> a prefix of P = 842 rows
(`<lidar_start>`, 840 prompt rows, `<lidar_end>`), then 20 .. 60 rows of question text (character tokenizer).  4 scenes x 8 questions,
greedy, no EOS, max_new_tokens 4 and 64, bf16x3 and bf16.

Method: every (mode, max_new_tokens, variant) is warmed up with a full run, then timed `--reps` times with the variants ALTERNATING in
this one process; a time is a host clock around work that ends in torch.cuda.synchronize(); the median is reported and min / max kept.
The batch_size = 1 and batch_size = 8 variants run code this feature does not touch (`prefix=None` takes the earlier path unchanged), so
they STAND IN for a separate build of the parent commit: a substitution, not a second build.  "share_scenes_interleaved" is the same
work with the scenes interleaved in the input, so that every group mixes all four scenes.  No profiler.  Also, per mode: ms of one
prefix prefill, of the question prefill of a group of 8, and of one decode step of 8 sequences -- the shared step
(lvq_qwen2_extend_shared, lq = 1) against the ragged step (lvq_qwen2_decode_step_ragged) on caches that hold prefix and own rows,
alternating, with the spread of each over the repetitions.

    python tools/bench_scene_prefix.py [--out profiles/scene_prefix.json] [--reps 3] [--layers 24]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lidar_vision_vqa_amd import _ffi as F, engine, fusion, head, ops, synth  # noqa: E402

GEO = dict(vocab=8192, d=896, inter=4864, n_heads=14, n_kv_heads=2, n_layers=24)
NQ, SCENES, PER_SCENE, GROUP = 840, 4, 8, 8
WORDS = "is the a car truck bus lane left right ahead behind near junction how many where cyclist pedestrian safe to turn stop go".split()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def med(xs):
    return dict(median_s=statistics.median(xs), min_s=min(xs), max_s=max(xs), spread=(max(xs) - min(xs)) / statistics.median(xs))


def questions():
    """32 questions of 20 .. 60 characters, seeded"""
    g = torch.Generator().manual_seed(3)
    out = []
    for i in range(SCENES * PER_SCENE):
        want = 20 + int(torch.randint(0, 41, (1,), generator=g))
        q = ""
        while len(q) < want:
            q += WORDS[int(torch.randint(0, len(WORDS), (1,), generator=g))] + " "
        out.append(q[:want - 1] + "?")
    return out


def answer_copy(eng, pairs, k):
    """The alternative to reading the prefix in place: the cached prefix rows are copied into per-question caches [B, P + Lq + k, dkv],
    the question rows are prefilled behind them with the generic attention kernel, and the tokens come from the ragged step."""
    base, dev = eng.base_model, eng.device
    c = base.cfg
    embs = [sc.question_rows(q) for sc, q in pairs]
    B, d, P = len(embs), c["d"], pairs[0][0].n_rows
    lens = torch.tensor([e.shape[1] for e in embs], dtype=torch.int32, device=dev)
    width = max(e.shape[1] for e in embs)
    x = torch.zeros((B, width, d), device=dev)
    for i, e in enumerate(embs):
        x[i, :e.shape[1]] = e[0]
    dkv, split, lmax = base.dh * c["n_kv_heads"], base._split(), P + width + k
    mk = lambda: (torch.empty((B, lmax, dkv), dtype=torch.bfloat16, device=dev),
                  torch.empty((B, lmax, dkv), dtype=torch.bfloat16, device=dev) if split else None)
    cache = [(mk(), mk()) for _ in base.model.layers]
    for i, layer in enumerate(cache):
        for kv in (0, 1):
            for part in ((0, 1) if split else (0,)):
                for b, (sc, _) in enumerate(pairs):
                    layer[kv][part][b, :P] = sc.prefix.layers[i][kv][part][0, :P]
    h = base._layers(x.view(B * width, d), B, width, P, cache)
    logits = base._logits(h.view(B, width, d)[torch.arange(B, device=dev), lens.long() - 1].contiguous())
    lib = F.lib()
    arr, keep = base._native_layers(cache)
    prec = 3 if split else 1
    geo = (F.cint(B), F.cint(d), F.cint(c["n_heads"]), F.cint(c["n_kv_heads"]), F.cint(c["inter"]))
    ws = torch.empty(int(lib.lvq_qwen2_decode_ragged_workspace_bytes(*geo, F.cint(lmax), F.cint(prec))), dtype=torch.uint8, device=dev)
    pos0 = (lens + P).contiguous()
    ids = []
    for t in range(k):
        nxt = ops.argmax_rows(logits)
        ids.append(nxt)
        if t + 1 == k:
            break
        xs = base.embed(nxt).float().contiguous()
        F.check(lib.lvq_qwen2_decode_step_ragged(arr, F.cint(len(base.model.layers)), F.ptr(xs), *geo, F.ptr(pos0), F.cint(t), F.cint(lmax),
                                                 F.cfloat(c["rms_eps"]), F.cfloat(c["rope_theta"]), F.cint(prec), F.ptr(ws),
                                                 F.csize(ws.numel()), F.stream_ptr(dev)), "lvq_qwen2_decode_step_ragged")
        logits = base._logits(xs)
    return eng._decode_rows(torch.stack(ids, dim=1))


def copy_variant(eng, qs, bevs, toks, k):
    scenes, pairs = {}, []
    for q, b, t in zip(qs, bevs, toks):
        if t not in scenes:
            scenes[t] = eng.open_scene(b, t)
        pairs.append((scenes[t], q))
    out = []
    for i in range(0, len(pairs), GROUP):
        out += answer_copy(eng, pairs[i:i + GROUP], k)
    return out


def bench_answers(eng, qs, bevs, toks, reps, mode):
    rows = []
    order = [s * PER_SCENE + j for j in range(PER_SCENE) for s in range(SCENES)]
    interleaved = ([qs[i] for i in order], [bevs[i] for i in order], [toks[i] for i in order])
    variants = {
        "batch_size_1": lambda k: eng.generate_batch(qs, bevs, toks, max_new_tokens=k, do_sample=False),
        "batch_size_8": lambda k: eng.generate_batch(qs, bevs, toks, GROUP, max_new_tokens=k, do_sample=False),
        "share_scenes": lambda k: eng.generate_batch(qs, bevs, toks, GROUP, share_scenes=True, max_new_tokens=k, do_sample=False),
        "copy_prefix_ragged_step": lambda k: copy_variant(eng, qs, bevs, toks, k),
        # the same triples with the scenes INTERLEAVED (scene 0, 1, 2, 3, 0, ...): every group of 8 mixes all four scenes, so every
        # generate call stacks four prefix caches (engine._stack_prefixes: row copies) and all scenes stay open to the end
        "share_scenes_interleaved": lambda k: eng.generate_batch(*interleaved, GROUP, share_scenes=True, max_new_tokens=k, do_sample=False),
    }
    for k in (4, 64):
        answers = {name: fn(k) for name, fn in variants.items()}                  # warm-up: every shape of the timed window
        t = {name: [] for name in variants}
        for _ in range(reps):
            for name, fn in variants.items():                                     # alternating
                t[name].append(timed(lambda: fn(k)))
        row = dict(mode=mode, max_new_tokens=k, answers=len(qs))
        for name in variants:
            m = med(t[name])
            ref = [answers["batch_size_1"][i] for i in order] if name == "share_scenes_interleaved" else answers["batch_size_1"]
            row[name] = dict(total=m, answers_per_s=len(qs) / m["median_s"],
                             same_answers_as_batch_size_1=sum(a == b for a, b in zip(answers[name], ref)))
        for name in ("batch_size_8", "share_scenes", "copy_prefix_ragged_step", "share_scenes_interleaved"):
            row[name + "_over_batch_size_1"] = row[name]["answers_per_s"] / row["batch_size_1"]["answers_per_s"]
        row["share_scenes_over_batch_size_8"] = row["share_scenes"]["answers_per_s"] / row["batch_size_8"]["answers_per_s"]
        row["share_scenes_over_copy"] = row["share_scenes"]["answers_per_s"] / row["copy_prefix_ragged_step"]["answers_per_s"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def bench_pieces(eng, qs, bevs, reps, mode, steps=200):
    """ms of the pieces, 8 questions of one scene: prefix prefill, question prefill, one decode step (shared against ragged)."""
    base, dev = eng.base_model, eng.device
    c = base.cfg
    scene = eng.open_scene(bevs[0], "piece")
    P, B, d = scene.n_rows, GROUP, c["d"]
    embs = [scene.question_rows(q) for q in qs[:B]]
    lens = torch.tensor([e.shape[1] for e in embs], dtype=torch.int32, device=dev)
    width = max(e.shape[1] for e in embs)
    rest = torch.zeros((B, width, d), device=dev)
    for i, e in enumerate(embs):
        rest[i, :e.shape[1]] = e[0]
    whole = torch.zeros((B, P + width, d), device=dev)
    for i, e in enumerate(embs):
        whole[i, :P], whole[i, P:P + e.shape[1]] = scene.rows[0], e[0]
    kw = dict(max_new_tokens=1, do_sample=False)
    calls = {
        "lidar_encoder_one_scene": lambda: eng.process_lidar(bevs[0]),
        "prefix_prefill_one_scene": lambda: base.prefill_prefix(scene.rows),
        "question_prefill_and_first_token_8_shared": lambda: base.generate(inputs_embeds=rest, prompt_lengths=lens, prefix=scene.prefix, **kw),
        "whole_prompt_prefill_and_first_token_8_ragged": lambda: base.generate(inputs_embeds=whole, prompt_lengths=lens + P, **kw),
    }
    out = {}
    for fn in calls.values():
        fn()
    t = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            t[name].append(timed(fn))
    for name in calls:
        m = med(t[name])
        out[name] = dict(ms=m["median_s"] * 1e3, min_ms=m["min_s"] * 1e3, max_ms=m["max_s"] * 1e3)
    # one decode step of 8 sequences, 24 layers: the shared step on (prefix, own) against the ragged step on caches that hold both
    lib, split = F.lib(), base._split()
    prec, dkv, own, lown = 3 if split else 1, base.dh * c["n_kv_heads"], 100, 100 + steps + 1
    mk = lambda rows: (torch.randn((B, rows, dkv), device=dev).to(torch.bfloat16),
                       torch.randn((B, rows, dkv), device=dev).to(torch.bfloat16) * 2.0 ** -9 if split else None)
    own_cache = [(mk(lown), mk(lown)) for _ in base.model.layers]
    cat_cache = [(mk(P + lown), mk(P + lown)) for _ in base.model.layers]
    arr_s, keep_s = base._native_layers(own_cache)
    arr_r, keep_r = base._native_layers(cat_cache)
    parr = (head._Qwen2PrefixPtrs * len(base.model.layers))()
    for i, ((kh, kl), (vh, vl)) in enumerate(scene.prefix.layers):
        parr[i] = head._Qwen2PrefixPtrs(kh.data_ptr(), None if kl is None else kl.data_ptr(), vh.data_ptr(), None if vl is None else vl.data_ptr())
    n_layers = F.cint(len(base.model.layers))
    geo = (F.cint(d), F.cint(c["n_heads"]), F.cint(c["n_kv_heads"]), F.cint(c["inter"]))
    ws_s = torch.empty(int(lib.lvq_qwen2_extend_shared_workspace_bytes(F.cint(B), F.cint(1), *geo, F.cint(P), F.cint(lown), F.cint(prec))),
                       dtype=torch.uint8, device=dev)
    ws_r = torch.empty(int(lib.lvq_qwen2_decode_ragged_workspace_bytes(F.cint(B), *geo, F.cint(P + lown), F.cint(prec))), dtype=torch.uint8, device=dev)
    pidx, ones = torch.zeros(B, dtype=torch.int32, device=dev), torch.ones(B, dtype=torch.int32, device=dev)
    own0 = torch.full((B,), own, dtype=torch.int32, device=dev) - torch.arange(B, dtype=torch.int32, device=dev)
    pos0 = (own0 + P).contiguous()
    x = 0.02 * torch.randn((B, d), device=dev)
    tail = (F.cfloat(c["rms_eps"]), F.cfloat(c["rope_theta"]), F.cint(prec))
    st = F.stream_ptr(dev)

    def shared():
        for t_ in range(steps):
            F.check(lib.lvq_qwen2_extend_shared(arr_s, parr, n_layers, F.ptr(x), F.cint(B), F.cint(1), *geo, F.ptr(pidx), F.ptr(scene.prefix.plen),
                                                F.cint(1), F.cint(P), F.ptr(own0), F.ptr(ones), F.cint(t_), F.cint(lown), *tail, F.ptr(ws_s),
                                                F.csize(ws_s.numel()), st), "lvq_qwen2_extend_shared")

    def ragged():
        for t_ in range(steps):
            F.check(lib.lvq_qwen2_decode_step_ragged(arr_r, n_layers, F.ptr(x), F.cint(B), *geo, F.ptr(pos0), F.cint(t_), F.cint(P + lown), *tail,
                                                     F.ptr(ws_r), F.csize(ws_r.numel()), st), "lvq_qwen2_decode_step_ragged")
    shared(), ragged()
    ts, tr = [], []
    for _ in range(max(reps, 5)):
        tr.append(timed(ragged) / steps * 1e3)
        ts.append(timed(shared) / steps * 1e3)
    ms, mr = statistics.median(ts), statistics.median(tr)
    out["decode_step_8_sequences"] = dict(shared_ms=ms, shared_min_ms=min(ts), shared_max_ms=max(ts), ragged_ms=mr, ragged_min_ms=min(tr),
                                          ragged_max_ms=max(tr), ragged_spread=(max(tr) - min(tr)) / mr, shared_over_ragged=ms / mr,
                                          shared_no_slower_beyond_ragged_spread=bool(ms <= mr + (max(tr) - min(tr))),
                                          prefix_rows=P, own_rows=f"{own - B + 1}..{own} + step", steps_per_repetition=steps)
    out["mode"] = mode
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_prefix.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=GEO["n_layers"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_prefix.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    GEO["n_layers"] = a.layers
    torch.manual_seed(0)
    base = head.StandInHead(GEO["vocab"], GEO["d"], GEO["inter"], GEO["n_heads"], GEO["n_kv_heads"], GEO["n_layers"]).to(dev).eval()
    vl = fusion.VATLiDAR(64, GEO["d"], NQ, 2, GEO["n_heads"]).to(dev).eval()
    eng = engine.InferenceEngine(dict(tokenizer=synth.DummyTokenizer(GEO["vocab"]), base_model=base, vat_lidar=vl, device=dev, d_model=GEO["d"],
                                      config=dict(use_vision=False, prefix_scale=0.2)))
    scene_bevs = [torch.randn((64, 32, 32), device=dev) for _ in range(SCENES)]
    qs = questions()
    bevs = [scene_bevs[i // PER_SCENE] for i in range(len(qs))]
    toks = [f"scene-{i // PER_SCENE}" for i in range(len(qs))]
    answers, pieces = [], []
    for mode in ("bf16x3", "bf16"):
        base.precision = vl.precision = mode
        pieces.append(bench_pieces(eng, qs, bevs, a.reps, mode))
        answers += bench_answers(eng, qs, bevs, toks, a.reps, mode)
    doc = dict(tool="tools/bench_scene_prefix.py", device=torch.cuda.get_device_name(0), hip=torch.version.hip, torch=torch.__version__,
               geometry=GEO, lidar=dict(c_in=64, canvas=[32, 32], n_queries=NQ, n_layers=2), prefix_rows=NQ + 2, scenes=SCENES,
               questions_per_scene=PER_SCENE, question_rows=[len(q) + len("\nAnswer:") for q in qs], reps=a.reps,
               timing="host clock around torch.cuda.synchronize(); median of reps; variants alternate", profiler="off",
               baseline="batch_size_1 / batch_size_8 run the code path the parent commit has, unchanged, in the same process",
               answers=answers, pieces=pieces)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
