#!/usr/bin/env python3
"""Decode throughput of a batch of questions: the per-question loop (one `generate` per prompt, what `generate_batch` does at
batch_size = 1) against ONE ragged `generate(..., prompt_lengths=)` call (csrc/decode_ragged.hip).

Geometry: Qwen2.5-0.5B as README quotes it (d 896, 14 / 2 heads, head_dim 64, inter 4864, 24 layers), random weights, vocabulary CUT
to 8192 rows (the lm head is outside the decode step and is the same work in both variants).  Prompts: random embeddings of unequal
length around the reference's real prefix (576 vision + 256 LiDAR rows + text: 880 rows, then 13 fewer per sequence); 64 new tokens,
greedy, no EOS.

Method: every (batch, mode, variant) is warmed up with a full run, then timed `--reps` times with the two variants ALTERNATING in this
one process; a time is a host clock around work that ends in torch.cuda.synchronize(); the median is reported and the spread kept.
ms per decode step = (time of 64 new tokens - time of 1 new token) / 63, i.e. without the prefill.  No profiler.  Also: the ragged
attention kernel pair against the generic tile kernel at batch 1 / 870 keys (device events), and the ragged step against the
scalar-position step on a uniform batch.

    python tools/bench_decode_batch.py [--out profiles/decode_ragged.json] [--reps 3] [--batches 1,2,4,8,16]
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
from lidar_vision_vqa_amd import _ffi as F, head, ops  # noqa: E402

GEO = dict(vocab=8192, d=896, inter=4864, n_heads=14, n_kv_heads=2, n_layers=24)
NEW, L0, LSTEP = 64, 880, 13


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def med(xs):
    return dict(median_s=statistics.median(xs), min_s=min(xs), max_s=max(xs))


def bench_generate(base, dev, batches, reps):
    out = []
    g = torch.Generator(device=dev).manual_seed(1)
    for n in batches:
        lens = [L0 - LSTEP * i for i in range(n)]
        singles = [0.02 * torch.randn((1, m, GEO["d"]), device=dev, generator=g) for m in lens]
        batch = torch.zeros((n, L0, GEO["d"]), device=dev)
        for i, s in enumerate(singles):
            batch[i, :s.shape[1]] = s[0]
        pl = torch.tensor(lens, dtype=torch.int32, device=dev)
        kw = dict(do_sample=False, eos_token_id=None)
        variants = {
            "loop": lambda k: [base.generate(inputs_embeds=s, max_new_tokens=k, **kw) for s in singles],
            "ragged": lambda k: base.generate(inputs_embeds=batch, prompt_lengths=pl, max_new_tokens=k, **kw),
        }
        if n == 8:      # the scalar-position step against the ragged step on the same uniform batch
            uni = 0.02 * torch.randn((n, L0 - 10, GEO["d"]), device=dev, generator=g)
            upl = torch.full((n,), L0 - 10, dtype=torch.int32, device=dev)
            variants["uniform_scalar"] = lambda k: base.generate(inputs_embeds=uni, max_new_tokens=k, **kw)
            variants["uniform_ragged"] = lambda k: base.generate(inputs_embeds=uni, prompt_lengths=upl, max_new_tokens=k, **kw)
        for mode in ("bf16x3", "bf16"):
            base.precision = mode
            for fn in variants.values():          # warm-up: every shape of the timed window
                fn(NEW)
            t = {name: {NEW: [], 1: []} for name in variants}
            for _ in range(reps):
                for k in (NEW, 1):
                    for name, fn in variants.items():     # alternating
                        t[name][k].append(timed(lambda: fn(k)))
            row = dict(batch=n, mode=mode, prompt_lengths=lens, new_tokens=NEW)
            for name in variants:
                full, first = med(t[name][NEW]), med(t[name][1])
                row[name] = dict(total=full, prefill_and_first_token=first,
                                 ms_per_decode_step=(full["median_s"] - first["median_s"]) / (NEW - 1) * 1e3,
                                 answers_per_s=n / full["median_s"])
            row["ragged_over_loop_answers_per_s"] = row["ragged"]["answers_per_s"] / row["loop"]["answers_per_s"]
            if n == 8:
                row["uniform_ragged_step_over_scalar_step"] = row["uniform_ragged"]["ms_per_decode_step"] / row["uniform_scalar"]["ms_per_decode_step"]
            print(json.dumps({k: v for k, v in row.items() if k != "prompt_lengths"}), flush=True)
            out.append(row)
    return out


def bench_attention(dev, iters=300):
    """batch 1, 870 keys, 14 / 2 heads of 64: lvq_attention_decode_ragged (both launches) and lvq_attention_bf16 with one query."""
    H, Hk, dh, nkv, lmax = 14, 2, 64, 870, 944
    res = {}
    for split in (True, False):
        q = ops.cast(torch.randn(1, H * dh, device=dev), split)
        kc = ops.cast(torch.randn(lmax, Hk * dh, device=dev), split)
        vc = ops.cast(torch.randn(lmax, Hk * dh, device=dev), split)
        kv_len = torch.tensor([nkv], dtype=torch.int32, device=dev)
        cs = (lmax * Hk * dh, Hk * dh, dh)
        st = (H * dh, H * dh, dh)
        calls = {
            "ragged_pair_us": lambda: ops.attention_decode_ragged(q, kc, vc, kv_len, batch=1, n_heads=H, n_kv_heads=Hk, lmax=lmax, dh=dh,
                                                                   q_strides=st, k_strides=cs, v_strides=cs, scale=dh ** -0.5),
            "tile_path_us": lambda: ops.attention(q, kc, vc, batch=1, n_heads=H, n_kv_heads=Hk, nq=1, nkv=nkv, dh=dh, q_strides=st,
                                                  k_strides=cs, v_strides=cs, scale=dh ** -0.5),
        }
        r = {}
        for _ in range(2):                         # alternating, second pass kept
            for name, fn in calls.items():
                for _ in range(20):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                r[name] = e0.elapsed_time(e1) / iters * 1e3
        res["bf16x3" if split else "bf16"] = r
    res["note"] = ("device-event time per call over back-to-back calls issued from Python: a floor set by the host's launch rate when the "
                   "kernels are shorter than a ctypes call; kernel times proper come from rocprofv3 --kernel-trace --stats")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_ragged.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="1,2,4,8,16")
    ap.add_argument("--layers", type=int, default=GEO["n_layers"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_batch.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    GEO["n_layers"] = a.layers
    torch.manual_seed(0)
    base = head.StandInHead(GEO["vocab"], GEO["d"], GEO["inter"], GEO["n_heads"], GEO["n_kv_heads"], GEO["n_layers"]).to(dev).eval()
    rows = bench_generate(base, dev, [int(x) for x in a.batches.split(",")], a.reps)
    att = bench_attention(dev)
    print(json.dumps(att), flush=True)
    doc = dict(tool="tools/bench_decode_batch.py", device=torch.cuda.get_device_name(0), hip=torch.version.hip, torch=torch.__version__,
               geometry=GEO, new_tokens=NEW, reps=a.reps, timing="host clock around torch.cuda.synchronize(); median of reps; variants alternate",
               profiler="off", generate=rows, attention_batch1_870_keys=att)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
