#!/usr/bin/env python3
"""Timing of VoxelResBackBone8xVoxelNeXt.forward at the reference's grid (0.075 m voxels, 41 x 1440 x 1440) on one and on eight
32 768-point Dist-C scenes, next to the voxeliser that feeds it.  Report only: nobody has measured this path before, there is no target.

Per layer (one `lvq_sparse_conv` launch each, BatchNorm / ReLU / residual fused): rows in and out, the active (row, offset) pairs, the
executed FLOPs 2 * pairs * C_in * C_out (x 3 in the hi + lo form, which runs three MFMA passes) and their share of the dense bf16 MFMA
peak over the time between two device events around the launch.  `rules_ms` is the time of the lvq_sparse_conv_rules calls (one per
indice_key, with one host read of the row count for layers that change the active set).  The total is a host clock around whole forwards
that end in a device synchronise; per-layer events are taken in a run of their own (they add host work between launches).

    python tools/bench_backbone3d.py [--iters 20] [--warmup 3] [--out profiles/backbone3d.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lidar_vision_vqa_amd import backbone3d as B3, lidar, synth  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0          # dense bf16 MFMA peak of the MI355X (never the 2:1-sparse figure)
RNG_VN, VS_VN = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], (0.075, 0.075, 0.2)


def scenes(n_scenes, n_points, dev):
    per = []
    for s in range(n_scenes):
        p = synth.scene_points("C", n_points, 2000 + s)
        p[:, :2] *= np.float32(54.0 / 51.2)
        per.append(p)
    pts = torch.from_numpy(np.concatenate(per)).to(dev)
    off = torch.tensor(np.concatenate(([0], np.cumsum([len(p) for p in per]))), dtype=torch.int32, device=dev)
    return pts, off


def named_convs(model):
    return {m: name for name, m in model.named_modules() if isinstance(m, B3._SparseConv)}


def measure(model, mode, n_scenes, n_points, iters, warmup, dev):
    pts, off = scenes(n_scenes, n_points, dev)
    gen = lidar.VoxelGeneratorWrapper(VS_VN, RNG_VN, 4, 10, 120000)

    def voxelise():
        feats, coords, num, svo = gen.generate_mean_device(pts, off, n_scenes)
        return feats, coords, svo

    feats, coords, svo = voxelise()
    m = int(svo[-1].item())
    bd = dict(voxel_features=feats[:m].contiguous(), voxel_coords=coords[:m].contiguous(), batch_size=n_scenes)
    model.precision = mode

    def forward():
        with torch.no_grad():
            return model(dict(bd))

    def host_ms(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3

    total_ms = host_ms(forward)
    voxel_ms = host_ms(voxelise)

    # per-layer events, in a run of their own
    names = named_convs(model)
    rec, rules_ev = {}, []
    real_run, real_rules = B3._SparseConv.run, B3.sparse_conv_rules

    def run(self, x, *a, **k):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n_rules = len(rules_ev)
        s.record()
        out = real_run(self, x, *a, **k)
        e.record()
        tab = out.indice_dict.get(self.indice_key if self.indice_key is not None else self)
        rec.setdefault(names[self], []).append((s, e, len(rules_ev) > n_rules, x.features.shape[0], out.features.shape[0], tab, self))
        return out

    def rules(*a, **k):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = real_rules(*a, **k)
        e.record()
        rules_ev.append((s, e))
        return out

    B3._SparseConv.run, B3.sparse_conv_rules = run, rules
    try:
        for _ in range(warmup + iters):
            forward()
        torch.cuda.synchronize()
    finally:
        B3._SparseConv.run, B3.sparse_conv_rules = real_run, real_rules
    layers = []
    passes = 3 if mode == "bf16x3" else 1
    n_fwd = warmup + iters
    for name, calls in rec.items():
        calls = calls[-iters:]
        with_rules = calls[-1][2]
        ms = float(np.mean([s.elapsed_time(e) for s, e, *_ in calls]))
        _, _, _, n_in, n_out, tab, conv = calls[-1]
        pairs = int((tab["nbr"] >= 0).sum().item())
        flops = 2 * pairs * conv.in_channels * conv.out_channels * passes
        entry = {"layer": name, "rows_in": n_in, "rows_out": n_out, "pairs": pairs, "c_in": conv.in_channels, "c_out": conv.out_channels,
                 "ms": round(ms, 4), "includes_rules": bool(with_rules), "gflop_executed": round(flops / 1e9, 3)}
        if not with_rules:
            entry["tflops"] = round(flops / ms / 1e9, 2)
            entry["frac_of_bf16_peak"] = round(flops / ms / 1e9 / PEAK_BF16_TFLOPS, 5)
        layers.append(entry)
    per_fwd = len(rules_ev) // n_fwd
    rules_ms = float(np.sum([s.elapsed_time(e) for s, e in rules_ev[-iters * per_fwd:]])) / iters
    flops_all = sum(l["gflop_executed"] for l in layers)
    return {"scenes": n_scenes, "points_per_scene": n_points, "voxels": m, "mode": mode, "forward_ms": round(total_ms, 3),
            "voxelise_mean_ms": round(voxel_ms, 3), "rules_ms": round(rules_ms, 3), "rules_calls": per_fwd,
            "gflop_executed": round(flops_all, 2), "forward_tflops": round(flops_all / total_ms, 2),
            "forward_frac_of_bf16_peak": round(flops_all / total_ms / PEAK_BF16_TFLOPS, 5), "layers": layers}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=32768)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_backbone3d.py needs an MI355X: there is no CPU timing of this path")
    dev = torch.device("cuda:0")
    grid = lidar.grid_size_from(RNG_VN, VS_VN).tolist()
    model = synth.load_seeded(B3.VoxelResBackBone8xVoxelNeXt({}, 4, grid), 6).to(dev).eval()
    res = {"what": "VoxelResBackBone8xVoxelNeXt.forward, Dist-C scenes stretched to +-54 m, grid 41 x 1440 x 1440", "device": torch.cuda.get_device_name(0),
           "peak_bf16_tflops": PEAK_BF16_TFLOPS, "iters": a.iters, "warmup": a.warmup, "runs": []}
    for n_scenes in (1, 8):
        for mode in ("bf16x3", "bf16"):
            r = measure(model, mode, n_scenes, a.points, a.iters, a.warmup, dev)
            res["runs"].append(r)
            print(f"{n_scenes} scene(s) {mode}: {r['voxels']} voxels, forward {r['forward_ms']:.3f} ms (rules {r['rules_ms']:.3f} ms in {r['rules_calls']} calls), "
                  f"voxelise+mean {r['voxelise_mean_ms']:.3f} ms, {r['gflop_executed']:.1f} GFLOP executed = {r['forward_frac_of_bf16_peak'] * 100:.2f} % of the bf16 peak",
                  flush=True)
            for l in r["layers"]:
                print(f"    {l['layer']:<22} {l['rows_in']:>7} -> {l['rows_out']:>7} rows, {l['pairs']:>9} pairs, {l['c_in']:>3} -> {l['c_out']:>3}: {l['ms']:.4f} ms"
                      + (f", {l['tflops']:.2f} TFLOP/s = {l['frac_of_bf16_peak'] * 100:.3f} % of peak" if "tflops" in l else " (with its rules call)"), flush=True)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
