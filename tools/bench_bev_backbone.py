#!/usr/bin/env python3
"""Timing of backbone2d.BaseBEVBackbone.forward (csrc/conv2d.hip) at the two nuScenes shapes of the reference's configs:
PointPillars (64 x 512 x 512 canvas, [3, 5, 5] layers, [64, 128, 256] filters, UPSAMPLE_STRIDES [0.5, 1, 2] -> 384 x 128 x 128) and SECOND
(256 x 128 x 128 canvas, [5, 5] layers, [128, 256] filters, [1, 2] -> 512 x 128 x 128), on one and on eight scenes, in both operand forms.
Report only: nobody has measured this path before, there is no reference number on this hardware and no target.

  forward_ms      device events around `iters` back-to-back forwards (to_planes included), divided by iters; `reps` such windows after a
                  warm-up of every shape: the median, with the smallest and largest window as the spread
  blocks          per block / deblock: device events around every lvq_conv2d / lvq_deconv2d launch, in a run of their own (the events add
                  host work between launches), summed per block; executed FLOPs 2 * pixels_out * taps * C_in * C_out (x 3 in the hi + lo
                  form, which runs three MFMA passes) and their share of the dense bf16 MFMA peak
  single_layer    one 3 x 3 stride-1 layer on an 8-scene 128 x 128 canvas, planes in and planes out, for the five (C_in, C_out) of the two
                  configs; next to it the same layer through backbone3d.SubMConv2d on the all-active grid (neighbour table built before
                  the window; the gather kernel stops at 128 channels) -- the only baseline that existed before this backbone

    python tools/bench_bev_backbone.py [--iters 40] [--reps 5] [--out profiles/bev_backbone.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lidar_vision_vqa_amd import backbone2d as B2, backbone3d as B3, synth  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0          # dense bf16 MFMA peak of the MI355X (never the 2:1-sparse figure)


class Cfg(dict):
    __getattr__ = dict.__getitem__


CONFIGS = {
    "nusc_pointpillars": (Cfg(LAYER_NUMS=[3, 5, 5], LAYER_STRIDES=[2, 2, 2], NUM_FILTERS=[64, 128, 256], UPSAMPLE_STRIDES=[0.5, 1, 2],
                              NUM_UPSAMPLE_FILTERS=[128, 128, 128]), (64, 512, 512)),
    "nusc_second": (Cfg(LAYER_NUMS=[5, 5], LAYER_STRIDES=[1, 2], NUM_FILTERS=[128, 256], UPSAMPLE_STRIDES=[1, 2],
                        NUM_UPSAMPLE_FILTERS=[256, 256]), (256, 128, 128)),
}
LAYER_SHAPES = ((64, 64), (64, 128), (128, 128), (128, 256), (256, 256))


def windows(fn, iters, reps, warmup=2):
    """ms per call over `reps` event-timed windows of `iters` calls: (median, min, max)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e) / iters)
    return float(np.median(out)), float(min(out)), float(max(out))


def layer_flops(layer, x, passes):
    oh, ow = layer.out_size(x.h, x.w, 1 if (not layer.transposed and layer.kernel == 3 and layer.padding == 0) else 0)
    taps = 1 if layer.transposed else layer.kernel ** 2
    return 2 * x.batch * oh * ow * taps * layer.c_in * layer.c_out * passes


def measure(model, name, shape, n_scenes, mode, iters, reps, dev):
    g = torch.Generator(device=dev).manual_seed(3000 + n_scenes)
    x = torch.randn((n_scenes,) + shape, device=dev, generator=g)
    x = x * (torch.rand((n_scenes, 1) + shape[1:], device=dev, generator=g) < 0.3)       # a scattered canvas: most pillars are empty
    model.precision = mode
    passes = 3 if mode == "bf16x3" else 1

    def forward():
        with torch.no_grad():
            return model(dict(spatial_features=x))["spatial_features_2d"]

    out = forward()
    med, lo, hi = windows(forward, iters, reps)
    # per-launch events, in a run of their own
    plan = model._plan()
    owner = {}
    for kind in ("blocks", "deblocks"):
        for i, layers in enumerate(plan[kind]):
            for layer, _ in layers:
                owner[layer] = f"{kind}.{i}"
    rec = {}
    real = B2._Layer.run

    def run(self, xin, *a, **k):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        res = real(self, xin, *a, **k)
        e.record()
        rec.setdefault(owner[self], []).append((s, e, layer_flops(self, xin, passes)))
        return res

    B2._Layer.run = run
    try:
        for _ in range(2 + iters):
            forward()
        torch.cuda.synchronize()
    finally:
        B2._Layer.run = real
    blocks, total_flops = [], 0
    for key, calls in rec.items():
        per = len(calls) // (2 + iters)
        calls = calls[2 * per:]
        ms = sum(s.elapsed_time(e) for s, e, _ in calls) / iters
        flops = sum(f for _, _, f in calls) / iters
        total_flops += flops
        blocks.append({"block": key, "launches": per, "ms": round(ms, 4), "gflop_executed": round(flops / 1e9, 2),
                       "tflops": round(flops / ms / 1e9, 1), "frac_of_bf16_peak": round(flops / ms / 1e9 / PEAK_BF16_TFLOPS, 4)})
    return {"config": name, "scenes": n_scenes, "mode": mode, "in": list(x.shape), "out": list(out.shape), "forward_ms": round(med, 3),
            "forward_ms_min": round(lo, 3), "forward_ms_max": round(hi, 3), "gflop_executed": round(total_flops / 1e9, 2),
            "forward_tflops": round(total_flops / med / 1e9, 1), "forward_frac_of_bf16_peak": round(total_flops / med / 1e9 / PEAK_BF16_TFLOPS, 4),
            "blocks": blocks}


def single_layers(iters, reps, dev):
    b, h, w = 8, 128, 128
    rows = []
    for cin, cout in LAYER_SHAPES:
        x = torch.from_numpy(synth.randn((b, cin, h, w), 4000 + cin)).to(dev)
        wt = torch.from_numpy(synth.randn((cout, cin, 3, 3), 4001 + cout, 1.0 / np.sqrt(9 * cin))).to(dev)
        conv = torch.nn.Conv2d(cin, cout, 3, padding=1, bias=False).to(dev)
        bn = torch.nn.BatchNorm2d(cout, eps=1e-3).to(dev).eval()
        with torch.no_grad():
            conv.weight.copy_(wt)
        layer = B2._Layer(conv, bn, True)
        row = {"c_in": cin, "c_out": cout, "grid": [b, h, w]}
        for mode in ("bf16x3", "bf16"):
            split = mode == "bf16x3"
            xp = B2.to_planes(x, split)
            dst = B2.Planes(b, h, w, cout, split, dev)
            med, lo, hi = windows(lambda: layer.run(xp, split, planes=dst), iters, reps)
            flops = 2 * b * h * w * 9 * cin * cout * (3 if split else 1)
            row[f"dense_{mode}_ms"] = [round(med, 4), round(lo, 4), round(hi, 4)]
            row[f"dense_{mode}_frac_of_bf16_peak"] = round(flops / med / 1e9 / PEAK_BF16_TFLOPS, 4)
        if cin <= 128 and cout <= 128:
            m = B3.SubMConv2d(cin, cout, 3, bias=False, indice_key="bench").to(dev).eval()
            bnd = torch.nn.BatchNorm1d(cout, eps=1e-3).to(dev).eval()
            idx = torch.stack(torch.meshgrid(torch.arange(b), torch.arange(h), torch.arange(w), indexing="ij"), dim=-1).reshape(-1, 3)
            feats = x.permute(0, 2, 3, 1).reshape(-1, cin).contiguous()
            with torch.no_grad():
                m.weight.copy_(wt.permute(0, 2, 3, 1))
                for mode in ("bf16x3", "bf16"):
                    st = B3.SparseConvTensor(feats, idx.to(torch.int32).to(dev).contiguous(), [h, w], b, None, mode)
                    m.run(st, bn=bnd, relu=True)                                # builds the neighbour table once; the window reuses it
                    med, lo, hi = windows(lambda: m.run(st, bn=bnd, relu=True), iters, reps)
                    row[f"submconv2d_{mode}_ms"] = [round(med, 4), round(lo, 4), round(hi, 4)]
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bev_backbone.py needs an MI355X: there is no CPU timing of this path")
    dev = torch.device("cuda:0")
    res = {"what": "BaseBEVBackbone.forward on lvq_conv2d / lvq_deconv2d; first measurement of this path, no reference number exists",
           "device": torch.cuda.get_device_name(0), "peak_bf16_tflops": PEAK_BF16_TFLOPS, "iters": a.iters, "reps": a.reps,
           "ms_fields": "median over reps windows; *_min / *_max or [median, min, max] give the spread", "runs": []}
    for name, (cfg, shape) in CONFIGS.items():
        model = synth.load_seeded(B2.BaseBEVBackbone(cfg, shape[0]), 9).to(dev).eval()
        for n_scenes in (1, 8):
            for mode in ("bf16x3", "bf16"):
                r = measure(model, name, shape, n_scenes, mode, a.iters, a.reps, dev)
                res["runs"].append(r)
                print(f"{name} x {n_scenes} {mode}: forward {r['forward_ms']:.3f} ms [{r['forward_ms_min']:.3f}, {r['forward_ms_max']:.3f}], "
                      f"{r['gflop_executed']:.1f} GFLOP executed = {r['forward_frac_of_bf16_peak'] * 100:.2f} % of the bf16 peak", flush=True)
                for bl in r["blocks"]:
                    print(f"    {bl['block']:<11} {bl['launches']} launches {bl['ms']:.4f} ms, {bl['tflops']:.1f} TFLOP/s = "
                          f"{bl['frac_of_bf16_peak'] * 100:.2f} % of peak", flush=True)
        del model
        torch.cuda.empty_cache()
    res["single_layer_3x3_stride1_8x128x128"] = single_layers(10 * a.iters, a.reps, dev)       # short kernels: longer windows
    for row in res["single_layer_3x3_stride1_8x128x128"]:
        print("   ", row, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
