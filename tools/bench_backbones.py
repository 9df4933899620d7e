#!/usr/bin/env python3
"""Timing of VoxelResBackBone8x (SECOND / CenterPoint) and PillarRes18BackBone8x (PillarNet) at the reference's nuScenes grid (0.075 m cells,
41 x 1440 x 1440 and 1440 x 1440) on one and on eight 32 768-point Dist-C scenes, in both precision modes, and of the 256 -> 256
submanifold layer of lvq_sparse_conv next to the 128 -> 128 instantiation on the same neighbour table.  Report only: nothing on this
path has a reference figure on this hardware.

Inputs: the voxels are those of tools/bench_backbone3d.py (hard voxeliser + mean); the pillars are the distinct (b, y, x) of those voxels
with seeded N(0, 1) features of 32 channels (what DynamicPillarVFESimple2D hands over in shape, not in value).
Forward time: a host clock around `iters` forwards that end in a device synchronise, repeated over `windows` windows after a warm-up:
median, min and max.  Per stage: device events around every launch, in a run of their own (they add host work between launches), summed
over the stage's layers; executed FLOPs are 2 * (row, offset) pairs * C_in * C_out per sparse layer (x 3 in the hi + lo form, which
runs three MFMA passes) and 2 * output pixels * 9 * C_in * C_out per dense layer.  `rules_ms` is the time inside lvq_sparse_conv_rules
calls (one per indice_key; a layer that changes the active set reads its row count on the host).

    python tools/bench_backbones.py [--iters 10] [--windows 5] [--warmup 3] [--out profiles/backbones_second_pillarnet.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_backbone3d as BB  # noqa: E402
from lidar_vision_vqa_amd import backbone2d as B2, backbone3d as B3, backbone_pillar as BP, lidar, synth  # noqa: E402

STAGES = ("conv_input", "conv1", "conv2", "conv3", "conv4", "conv_out", "conv5")


def spread(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(np.min(xs)), 4), "max": round(float(np.max(xs)), 4)}


def windows_ms(fn, iters, windows, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters * 1e3)
    return out


def inputs(n_scenes, n_points, dev):
    """(voxel batch_dict, pillar batch_dict) of the same scenes."""
    pts, off = BB.scenes(n_scenes, n_points, dev)
    gen = lidar.VoxelGeneratorWrapper(BB.VS_VN, BB.RNG_VN, 4, 10, 120000)
    feats, coords, num, svo = gen.generate_mean_device(pts, off, n_scenes)
    m = int(svo[-1].item())
    feats, coords = feats[:m].contiguous(), coords[:m].contiguous()
    pillars = torch.unique(coords[:, [0, 2, 3]], dim=0).to(torch.int32).contiguous()
    pf = torch.from_numpy(synth.randn((pillars.shape[0], 32), 77)).to(dev)
    return (dict(voxel_features=feats, voxel_coords=coords, batch_size=n_scenes),
            dict(pillar_features=pf, pillar_coords=pillars, batch_size=n_scenes))


def measure(model, bd, mode, iters, windows, warmup):
    model.precision = mode
    passes = 3 if mode == "bf16x3" else 1

    def forward():
        with torch.no_grad():
            return model(dict(bd))

    total = windows_ms(forward, iters, windows, warmup)
    names = {m: n for n, m in model.named_modules() if isinstance(m, (B3._SparseConv, torch.nn.Conv2d))}
    rec, rules_ev = {}, []
    real_run, real_rules, real_dense = B3._SparseConv.run, B3.sparse_conv_rules, B2._Layer.run

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(self, x, *a, **k):
        s, e = events()
        n_rules = len(rules_ev)
        s.record()
        out = real_run(self, x, *a, **k)
        e.record()
        tab = out.indice_dict.get(self.indice_key if self.indice_key is not None else self)
        flops = 2 * int((tab["nbr"] >= 0).sum().item()) * self.in_channels * self.out_channels * passes
        rec.setdefault(names[self], []).append((s, e, len(rules_ev) > n_rules, flops))
        return out

    def dense(self, x, split, pad=0, **k):
        s, e = events()
        s.record()
        out = real_dense(self, x, split, pad, **k)
        e.record()
        oh, ow = self.out_size(x.h, x.w, pad)
        rec.setdefault(names[self.conv], []).append((s, e, False, 2 * x.batch * oh * ow * self.kernel ** 2 * self.c_in * self.c_out * passes))
        return out

    def rules(*a, **k):
        s, e = events()
        s.record()
        out = real_rules(*a, **k)
        e.record()
        rules_ev.append((s, e))
        return out

    B3._SparseConv.run, B3.sparse_conv_rules, B2._Layer.run = run, rules, dense
    try:
        for _ in range(warmup + iters):
            forward()
        torch.cuda.synchronize()
    finally:
        B3._SparseConv.run, B3.sparse_conv_rules, B2._Layer.run = real_run, real_rules, real_dense
    stages = {}
    for name, calls in rec.items():
        calls = calls[-iters:]
        st = stages.setdefault(name.split(".")[0], {"ms": 0.0, "gflop_executed": 0.0, "launches": 0, "includes_rules": False})
        st["ms"] += float(np.mean([s.elapsed_time(e) for s, e, *_ in calls]))
        st["gflop_executed"] += calls[-1][3] / 1e9
        st["launches"] += 1
        st["includes_rules"] |= bool(calls[-1][2])
    per_fwd = len(rules_ev) // (warmup + iters)
    rules_ms = float(np.sum([s.elapsed_time(e) for s, e in rules_ev[-iters * per_fwd:]])) / iters
    gflop = sum(s["gflop_executed"] for s in stages.values())
    med = float(np.median(total))
    return {"mode": mode, "forward_ms": spread(total), "rules_ms": round(rules_ms, 3), "rules_calls": per_fwd, "rules_share": round(rules_ms / med, 3),
            "gflop_executed": round(gflop, 2), "forward_tflops": round(gflop / med, 2),
            "stages": {k: {kk: (round(v, 4) if isinstance(v, float) else v) for kk, v in stages[k].items()} for k in STAGES if k in stages}}


def wide_layer(table, n, mode, iters, windows, warmup, dev):
    """The 256 -> 256 and the 128 -> 128 submanifold 3 x 3 layer (conv + BatchNorm + ReLU in one launch) on ONE neighbour table."""
    out = {}
    for c in (128, 256):
        conv = synth.load_seeded(B3.SubMConv2d(c, c, 3, padding=1, bias=False, indice_key="t"), 5).to(dev).eval()
        bn = synth.load_seeded(torch.nn.BatchNorm1d(c, eps=1e-3), 6).to(dev).eval()
        x = B3.SparseConvTensor(torch.from_numpy(synth.randn((n, c), 7)).to(dev), table["in_indices"], table["out_shape"], 1, {"t": table}, mode)
        evs = []

        def one():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            with torch.no_grad():
                for _ in range(iters):
                    conv.run(x, bn=bn, relu=True)
            e.record()
            evs.append((s, e))

        for _ in range(warmup + windows):
            one()
        torch.cuda.synchronize()
        ms = [s.elapsed_time(e) / iters for s, e in evs[warmup:]]
        pairs = int((table["nbr"] >= 0).sum().item())
        flops = 2 * pairs * c * c * (3 if mode == "bf16x3" else 1)
        out[f"{c}->{c}"] = {"ms": spread(ms), "pairs": pairs, "rows": n, "gflop_executed": round(flops / 1e9, 3),
                            "tflops": round(flops / float(np.median(ms)) / 1e9, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=32768)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_backbones.py needs an MI355X: there is no CPU timing of this path")
    dev = torch.device("cuda:0")
    grid = lidar.grid_size_from(BB.RNG_VN, BB.VS_VN).tolist()
    models = {"VoxelResBackBone8x": synth.load_seeded(B3.VoxelResBackBone8x({}, 4, grid), 6).to(dev).eval(),
              "PillarRes18BackBone8x": synth.load_seeded(BP.PillarRes18BackBone8x({}, 32, grid), 6).to(dev).eval()}
    res = {"what": "VoxelResBackBone8x / PillarRes18BackBone8x forward, Dist-C scenes stretched to +-54 m, grid 41 x 1440 x 1440 / 1440 x 1440",
           "device": torch.cuda.get_device_name(0), "iters": a.iters, "windows": a.windows, "warmup": a.warmup, "runs": [], "wide_layer": {}}
    for n_scenes in (1, 8):
        vbd, pbd = inputs(n_scenes, a.points, dev)
        for name, bd in (("VoxelResBackBone8x", vbd), ("PillarRes18BackBone8x", pbd)):
            rows = int((bd.get("voxel_coords", bd.get("pillar_coords"))).shape[0])
            for mode in ("bf16x3", "bf16"):
                r = dict(backbone=name, scenes=n_scenes, rows_in=rows, **measure(models[name], bd, mode, a.iters, a.windows, a.warmup))
                res["runs"].append(r)
                f = r["forward_ms"]
                print(f"{name} {n_scenes} scene(s) {mode}: {rows} rows, forward {f['median']:.3f} ms (min {f['min']:.3f}, max {f['max']:.3f}), rules "
                      f"{r['rules_ms']:.3f} ms in {r['rules_calls']} calls, {r['gflop_executed']:.1f} GFLOP executed = {r['forward_tflops']:.2f} TFLOP/s end to end",
                      flush=True)
                for k, s in r["stages"].items():
                    print(f"    {k:<11} {s['launches']:>2} launches {s['ms']:.4f} ms, {s['gflop_executed']:.3f} GFLOP"
                          + (" (with its rules calls)" if s["includes_rules"] else f" = {s['gflop_executed'] / s['ms']:.2f} TFLOP/s"), flush=True)
        # the wide layer's yardstick: conv4's submanifold table of this batch of pillars
        m = models["PillarRes18BackBone8x"]
        with torch.no_grad():
            x3 = m.conv3(m.conv2(m.conv1(B3.SparseConvTensor(pbd["pillar_features"], pbd["pillar_coords"], m.sparse_shape, n_scenes, None, "bf16x3"))))
            x4 = m.conv4[0](x3)
            x4 = B3.SparseConvTensor(x4.features, x4.indices, x4.spatial_shape, n_scenes, {}, "bf16x3")
            m.conv4[1].conv1.run(x4)
        table = x4.indice_dict["res4"]
        for mode in ("bf16x3", "bf16"):
            w = wide_layer(table, x4.features.shape[0], mode, 20 * a.iters, a.windows, a.warmup, dev)
            res["wide_layer"][f"{n_scenes} scene(s) {mode}"] = w
            print(f"wide layer, {n_scenes} scene(s) {mode}: " + "; ".join(f"{k} {v['ms']['median']:.4f} ms (min {v['ms']['min']:.4f}, max {v['ms']['max']:.4f}) "
                                                                        f"{v['tflops']:.2f} TFLOP/s executed" for k, v in w.items()), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
