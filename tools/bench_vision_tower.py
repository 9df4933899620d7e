#!/usr/bin/env python3
"""Timing of vision_tower.ImageEncoderViT.forward (build_sam_vit_b, seeded weights) at 1024 x 1024 on one and on six images, in both
operand forms, and of the fused relative-position attention (csrc/vit_attention.hip) on its own.
Report only: nobody has measured this path before, there is no reference number on this hardware and no target.

  forward_ms       device events around `iters` back-to-back forwards, divided by iters; `reps` such windows after a warm-up of every
                   shape: the median, with the smallest and largest window as the spread
  kernels          per kind of launch (gemm, layernorm, cast, attention of the windowed / of the global blocks, conv2d): device events
                   around every call of the ops wrappers, in a run of their own (the events add host work between launches); `torch`
                   is the rest of the forward -- the copies of the patch gather, the window split and its inverse, the permutes
  attention        the two attention shapes of one image on their own (25 windows of 14 x 14, and one 64 x 64 grid, 12 heads): ms and
                   executed FLOPs -- 2 N^2 dh for the scores and the same for P V, per head, x 3 in the hi + lo form; the bias table
                   product (a few per cent on top) is not counted -- as a share of the dense bf16 MFMA peak
  dense_bias_route lvq_attention_bf16 (the parent's kernel) with the bias materialised as a dense fp32 [1, 12, 1024, 1024] array
                   (50 MB: a 32 x 32 grid, the largest shape at which that route is reasonable) against the fused kernel on the same
                   operands, in alternation, `reps` (>= 5) windows each: medians and spreads of both

    python tools/bench_vision_tower.py [--iters 10] [--reps 5] [--out profiles/vision_tower.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lidar_vision_vqa_amd import ops as O, synth, vision_tower as VT  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0          # dense bf16 MFMA peak of the MI355X (never the 2:1-sparse figure)
DH = 64


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def windows(fn, iters, reps, warmup=2):
    """ms per call over `reps` event-timed windows of `iters` calls: (median, min, max)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = [window(fn, iters) for _ in range(reps)]
    return float(np.median(out)), float(min(out)), float(max(out))


def attention_flops(batch, heads, gh, gw, passes):
    n = gh * gw
    return batch * heads * 4 * n * n * DH * passes


def split_by_kernel(forward, iters):
    """Device events around every wrapper call of one forward, summed per kind; a run of its own."""
    rec = {}

    def timed(name, fn):
        def run(*a, **k):
            kind = name if name != "attention" else ("attention_window" if k["gh"] == 14 else "attention_global")
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            res = fn(*a, **k)
            e.record()
            rec.setdefault(kind, []).append((s, e))
            return res
        return run

    saved = (O.linear, O.layernorm, O.cast, O.attention_relpos, VT._conv)
    O.linear, O.layernorm, O.cast, O.attention_relpos = (timed(n, f) for n, f in zip(("gemm", "layernorm", "cast", "attention"), saved[:4]))
    VT._conv = timed("conv2d", saved[4])
    try:
        for _ in range(2 + iters):
            forward()
        torch.cuda.synchronize()
    finally:
        O.linear, O.layernorm, O.cast, O.attention_relpos, VT._conv = saved
    out = {}
    for kind, calls in rec.items():
        per = len(calls) // (2 + iters)
        out[kind] = {"launches": per, "ms": round(sum(s.elapsed_time(e) for s, e in calls[2 * per:]) / iters, 4)}
    return out


def measure_forward(model, batch, mode, iters, reps, dev):
    x = torch.from_numpy(synth.randn((batch, 3, 1024, 1024), 5000 + batch)).to(dev)
    model.precision = mode

    def forward():
        with torch.no_grad():
            return model(x)

    out = forward()
    med, lo, hi = windows(forward, iters, reps)
    kinds = split_by_kernel(forward, iters)
    kinds["torch"] = {"launches": None, "ms": round(med - sum(v["ms"] for v in kinds.values()), 4)}
    return {"images": batch, "mode": mode, "in": list(x.shape), "out": list(out.shape), "forward_ms": round(med, 3), "forward_ms_min": round(lo, 3),
            "forward_ms_max": round(hi, 3), "kernels": kinds}


def attention_operands(batch, heads, gh, gw, split, dev, seed=6000):
    import vision_tower_cases as VC
    qkv, rh, rw = (torch.from_numpy(a).to(dev) for a in VC.kernel_operands(batch, heads, gh, gw, DH, seed))
    return tuple(O.cast(t, split) for t in (qkv, rh, rw))


def measure_attention(batch, heads, gh, gw, mode, iters, reps, dev):
    split = mode == "bf16x3"
    qkv, rh, rw = attention_operands(batch, heads, gh, gw, split, dev)
    fn = lambda: O.attention_relpos(qkv, rh, rw, batch=batch, n_heads=heads, gh=gh, gw=gw, dh=DH, scale=DH ** -0.5)
    med, lo, hi = windows(fn, iters, reps)
    flops = attention_flops(batch, heads, gh, gw, 3 if split else 1)
    return {"batch": batch, "heads": heads, "grid": [gh, gw], "mode": mode, "ms": [round(med, 4), round(lo, 4), round(hi, 4)],
            "gflop_executed": round(flops / 1e9, 2), "tflops": round(flops / med / 1e9, 1),
            "frac_of_bf16_peak": round(flops / med / 1e9 / PEAK_BF16_TFLOPS, 4)}


def dense_bias_route(mode, iters, reps, dev):
    """The parent's lvq_attention_bf16 with a dense fp32 bias against the fused kernel: 32 x 32 grid, 12 heads, batch 1, alternating."""
    import vision_tower_cases as VC
    g, heads, split = 32, 12, mode == "bf16x3"
    n, d = g * g, heads * DH
    qkv, rh, rw = attention_operands(1, heads, g, g, split, dev)
    q64 = (qkv[0].float() + (qkv[1].float() if split else 0)).cpu().numpy().reshape(1, n, 3, heads, DH)[:, :, 0].transpose(0, 2, 1, 3)
    tab = lambda t: (t[0].float() + (t[1].float() if split else 0)).cpu().numpy()
    bias = torch.from_numpy(VC.dense_bias(q64, tab(rh), tab(rw), g, g)).float().contiguous().to(dev)
    col = lambda t, i: None if t is None else t[:, i * d:(i + 1) * d]
    part = lambda i: (col(qkv[0], i), col(qkv[1], i))
    st = (n * 3 * d, 3 * d, DH)
    # the column slices are views: the wrapper passes their data pointers and the packed strides
    dense = lambda: O.attention(part(0), part(1), part(2), batch=1, n_heads=heads, n_kv_heads=heads, nq=n, nkv=n, dh=DH, q_strides=st,
                                k_strides=st, v_strides=st, scale=DH ** -0.5, bias=bias)
    fused = lambda: O.attention_relpos(qkv, rh, rw, batch=1, n_heads=heads, gh=g, gw=g, dh=DH, scale=DH ** -0.5)
    a, b = dense(), fused()
    agree = float(((a[0].float() + (a[1].float() if split else 0)) - (b[0].float() + (b[1].float() if split else 0))).abs().max())
    for _ in range(2):
        dense(), fused()
    torch.cuda.synchronize()
    td, tf = [], []
    for _ in range(max(5, reps)):
        td.append(window(dense, iters))
        tf.append(window(fused, iters))
    stat = lambda v: [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]
    return {"grid": [g, g], "heads": heads, "mode": mode, "bias_mb": round(bias.numel() * 4 / 1e6, 1), "dense_bias_ms": stat(td), "fused_ms": stat(tf),
            "fused_at_least_as_fast": bool(np.median(tf) <= np.median(td)), "max_abs_difference_of_outputs": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vision_tower.py needs an MI355X: there is no CPU timing of this path")
    dev = torch.device("cuda:0")
    res = {"what": "ImageEncoderViT.forward (SAM ViT-B, 1024 x 1024) on liblvq_hip.so; first measurement of this path, no reference number exists",
           "device": torch.cuda.get_device_name(0), "peak_bf16_tflops": PEAK_BF16_TFLOPS, "iters": a.iters, "reps": a.reps,
           "ms_fields": "median over reps windows; *_min / *_max or [median, min, max] give the spread", "forward": [], "attention": [],
           "dense_bias_route": []}
    model = synth.load_seeded(VT.build_sam_vit_b(), 9).to(dev).eval()
    for batch in (1, 6):
        for mode in VT.MODES:
            r = measure_forward(model, batch, mode, a.iters, a.reps, dev)
            res["forward"].append(r)
            print(f"{batch} x 1024^2 {mode}: forward {r['forward_ms']:.3f} ms [{r['forward_ms_min']:.3f}, {r['forward_ms_max']:.3f}]", flush=True)
            for k, v in r["kernels"].items():
                print(f"    {k:<17} {v['launches']} launches {v['ms']:.4f} ms", flush=True)
    del model
    torch.cuda.empty_cache()
    for batch, gh, gw in ((25, 14, 14), (1, 64, 64)):
        for mode in VT.MODES:
            r = measure_attention(batch, 12, gh, gw, mode, 10 * a.iters, a.reps, dev)
            res["attention"].append(r)
            print(f"attention {batch} x 12 x {gh} x {gw} {mode}: {r['ms']} ms, {r['tflops']} TFLOP/s = {r['frac_of_bf16_peak'] * 100:.2f} % of peak", flush=True)
    for mode in VT.MODES:
        r = dense_bias_route(mode, 10 * a.iters, a.reps, dev)
        res["dense_bias_route"].append(r)
        print(f"32 x 32 x 12 heads {mode}: dense-bias route {r['dense_bias_ms']} ms, fused {r['fused_ms']} ms, outputs differ by "
              f"{r['max_abs_difference_of_outputs']:.2e}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
