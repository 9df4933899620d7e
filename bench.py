#!/usr/bin/env python3
"""bench.py -- throughput of the LiDAR-vision fusion hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints ONE JSON line with the headline figure (`value` fused tokens/s,
`ms_per_step`); nothing else runs.  `--dump-outputs DIR` writes what the last timed step returned as DIR/<name>.npy (dump_outputs).
`--full` adds every secondary measurement and check described below to the same line.

A "step" is ONE pass of the hot path (lidar_vision_vqa_amd.pipeline.FusionPipeline) over one batch of `--scenes` synthetic
scenes per GPU (default 32): points and image-patch tokens are already resident in HBM when the timed region starts.
Workload = BASELINE.json configs[1]: 32 768-point Dist-C scenes, 0.1 m voxel grid, 196 ViT-B/16 patches,
d = 768, 12 heads, bf16 MFMA.  Scenes shard one batch per rank with no data-path collective; the only exchange is one RCCL
all-reduce(SUM) per step of a fused fp32 buffer [token-sum (d) | scene count] -> "scaling": "weak".

`--workload cfg4` / `cfg5` run BASELINE configs[3] / configs[4] instead (120 000-point scenes with max_voxels = 160 000; the token-level
VQA-head workload 256 LiDAR x 576 image x 32 answer tokens), both with the stand-in language head attached and the all-reduced buffer
[loss | n_scenes | answer-logit sums]; the default (cfg2) is the configuration the metric is quoted on.

`value` is measured in the precision mode `--precision` (default "mixed": bf16 MFMA tiles everywhere, plain bf16 operands on the
262 144-key K/V stream, hi + lo bf16 operands elsewhere -- the fastest mode that meets the north-star 1e-3 tolerance, see
`parity_vs_cpu` of a `--full` run, which is measured for EVERY mode timed there against the CPU oracle on three scenes).  With `--full`,
rank 0's line also holds `roofline` = the cross-attention kernel at the metric's own shape "32k pts x 196 patches" (lvq_ca_fused at (1, 32768, 196, 768, 12):
SURVEY 8d's algorithmic FLOPs / HIP-event time of its launches on the launch stream), `roofline_attention` = the dominant kernel of the
step (VATLiDAR's cross-attention over the BEV key stream; three readings of its FLOPs), `roofline_bev_kv`, every cross-attention row of
SURVEY 8d, the HBM-bound voxelisers at cfg-3, the same workload on Dist-U scenes and at the reference's default depth, and `cpu_baseline`
(the CPU restatement in oracle/ timed on the host cores on a bounded sample, thread count chosen by a sweep).
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

PEAK_BF16_TFLOPS = 2500.0   # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md (never the 2:1-sparse figure)
PEAK_HBM_GBS = 8000.0
TOL = 1e-3                  # north_star: fused tokens within 1e-3 of the fp32 CPU path
MODES = ("mixed", "mixed16", "bf16", "bf16x3")


def avg_ms(pairs):
    return float(np.mean([s.elapsed_time(e) for s, e in pairs])) if pairs else None


def event_ms(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def profile_traffic(prefixes):
    """HBM bytes per launch from the committed rocprofv3 --pmc passes (profiles/*pmc_traffic*.json; counters cannot be read from
    inside this process).  Returns (bytes | None, source file | None): a constant of the committed profile, not a live reading."""
    for name in sorted(os.listdir(os.path.join(ROOT, "profiles")), reverse=True):
        if "pmc_traffic" not in name or not name.endswith(".json"):
            continue
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                for k, v in json.load(f).items():
                    if any(k.startswith(p) for p in prefixes):
                        return v["traffic_bytes_per_launch"], "profiles/" + name
        except Exception:
            continue
    return None, None


def cross_attention_rows(P, fusion, dev, rows_filter=None):
    """Every cross-attention row of SURVEY 8d: the whole `q + ca(ca_ln(q), kv, kv)` sub-path, all modes."""
    rows = [("32k pts x 196 patches (headline)", 1, 32768, 196, 768, 12), ("resampled tokens x patches", 1, 576, 196, 768, 12),
            ("resampled tokens x patches, batch 8", 8, 576, 196, 768, 12), ("cfg-5", 8, 256, 576, 768, 12),
            ("reference-true VATLiDAR", 1, 576, 32400, 896, 8), ("reference-true VATVision", 1, 768, 1536, 2048, 8)]
    out = {}
    for label, B, nq, nkv, d, h in rows:
        if rows_filter and label not in rows_filter:
            continue
        blk = fusion.VATBlock(d, h, 4 * d, 0.1).to(dev).eval()
        q, kv = torch.randn(B, nq, d, device=dev), torch.randn(B, nkv, d, device=dev)
        flops = B * (4.0 * nq * d * d + 4.0 * nkv * d * d + 4.0 * nq * nkv * d)
        entry = {"shape": [B, nq, nkv, d, h], "flops": flops}
        for mode in MODES:
            blk.precision = mode
            ms = event_ms(lambda: blk.cross_attention(q, kv), iters=10)
            entry[mode] = {"ms": round(ms, 4), "tflops": round(flops / ms / 1e9, 1), "frac_of_bf16_peak": round(flops / ms / 1e9 / PEAK_BF16_TFLOPS, 4)}
        out[label] = entry
        del blk, q, kv
    return out


def voxel_blocks(dev):
    """HBM-bound side at BASELINE cfg-3 (8 scenes x 65 536 points, 0.1 m grid): hard and dynamic voxelisers, whole call.
    Algorithmic bytes: hard 16 N + M (4 T C + 16); dynamic 20 N + M * 16 + 4 N (unq_inv materialised)."""
    from lidar_vision_vqa_amd import lidar as LD, synth as SY
    scenes = [SY.scene_points("C", 65536, 1010 + i) for i in range(8)]
    lens = [len(x) for x in scenes]
    pts = torch.from_numpy(np.concatenate(scenes)).to(dev)
    off = torch.tensor(np.concatenate(([0], np.cumsum(lens))), dtype=torch.int32, device=dev)
    rng = list(SY.PC_RANGE_NUSC)
    gen = LD.VoxelGeneratorWrapper(SY.VOXEL_01, rng, 4, 10, 160000)
    m_vox = int(gen.generate_batch_device(pts, off, 8)[3][-1])
    us = event_ms(lambda: gen.generate_batch_device(pts, off, 8), iters=20) * 1e3
    nbytes = 16.0 * pts.shape[0] + m_vox * (4.0 * 10 * 4 + 16)
    tr, src = profile_traffic(["lvq_voxelize_hard (voxel_hashed.hip) 8 x 65536 points"])
    hard = {"bound": "hbm", "kernels": "lvq_voxelize_hard, whole call", "us": round(us, 1), "points": int(pts.shape[0]), "voxels": m_vox,
            "achieved": round(nbytes / us / 1e3, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(nbytes / us / 1e3 / PEAK_HBM_GBS, 4),
            "frac_of_6300_achievable": round(nbytes / us / 1e3 / 6300.0, 4), "algorithmic_bytes": nbytes, "traffic": tr, "traffic_source": src}
    us_m = event_ms(lambda: gen.generate_mean_device(pts, off, 8), iters=20) * 1e3
    nb_m = 16.0 * pts.shape[0] + m_vox * (4.0 * 4 + 16)
    mean = {"bound": "hbm", "kernels": "lvq_voxelize_mean (voxelise -> MeanVFE fused), whole call", "us": round(us_m, 1),
            "achieved": round(nb_m / us_m / 1e3, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(nb_m / us_m / 1e3 / PEAK_HBM_GBS, 4),
            "algorithmic_bytes": nb_m}
    bidx = torch.repeat_interleave(torch.arange(8, device=dev, dtype=torch.float32), torch.tensor(lens, device=dev))
    bp = torch.cat((bidx[:, None], pts), 1).contiguous()
    grid = LD.grid_size_from(rng, SY.VOXEL_01)
    m_dyn = int(LD._dynamic_voxelize(bp, 8, rng, SY.VOXEL_01, grid, 3)["counts"][0])
    us_d = event_ms(lambda: LD._dynamic_voxelize(bp, 8, rng, SY.VOXEL_01, grid, 3), iters=20) * 1e3
    nb_d = 20.0 * bp.shape[0] + 4.0 * bp.shape[0] + m_dyn * (4.0 + 4.0 + 16.0)       # points in, unq_inv, (key, count, coords) per voxel
    tr, src = profile_traffic(["lvq_voxelize_dynamic 8 x 65536 points"])
    dyn = {"bound": "hbm", "kernels": "lvq_voxelize_dynamic (unique keys ascending + inverse + counts + coords), whole call",
           "us": round(us_d, 1), "points": int(bp.shape[0]), "voxels": m_dyn, "achieved": round(nb_d / us_d / 1e3, 1), "peak": PEAK_HBM_GBS,
           "unit": "GB/s", "frac": round(nb_d / us_d / 1e3 / PEAK_HBM_GBS, 4), "algorithmic_bytes": nb_d, "traffic": tr, "traffic_source": src}
    return hard, mean, dyn, scenes


def voxel_scaling(dev):
    """The three voxelisers at sizes where bandwidth rather than the ~5 us floor of each dependent launch decides:
    cfg-3 (8 x 65 536), 32 x 65 536 and 8 x 120 000 points; whole call, HIP events, algorithmic bytes of SURVEY 8d."""
    from lidar_vision_vqa_amd import lidar as LD, synth as SY
    rng = list(SY.PC_RANGE_NUSC)
    grid = LD.grid_size_from(rng, SY.VOXEL_01)
    out = {}
    for label, ns, npts in (("8x65536", 8, 65536), ("32x65536", 32, 65536), ("8x120000", 8, 120000)):
        scenes = [SY.scene_points("C", npts, 1010 + i) for i in range(ns)]
        lens = [len(x) for x in scenes]
        pts = torch.from_numpy(np.concatenate(scenes)).to(dev)
        off = torch.tensor(np.concatenate(([0], np.cumsum(lens))), dtype=torch.int32, device=dev)
        gen = LD.VoxelGeneratorWrapper(SY.VOXEL_01, rng, 4, 10, 160000)
        m_vox = int(gen.generate_batch_device(pts, off, ns)[3][-1])
        n = float(pts.shape[0])
        us_h = event_ms(lambda: gen.generate_batch_device(pts, off, ns), iters=20) * 1e3
        us_m = event_ms(lambda: gen.generate_mean_device(pts, off, ns), iters=20) * 1e3
        entry = {"points": int(n), "voxels": m_vox}
        for name, us, nb in (("hard", us_h, 16.0 * n + m_vox * (4.0 * 10 * 4 + 16)), ("fused_mean", us_m, 16.0 * n + m_vox * (4.0 * 4 + 16))):
            entry[name] = {"us": round(us, 1), "GBps": round(nb / us / 1e3, 1), "frac": round(nb / us / 1e3 / PEAK_HBM_GBS, 4)}
        if ns * grid[0] * grid[1] * grid[2] < 2 ** 31:             # the dynamic voxeliser's int32 key space (scene index x cells)
            bidx = torch.repeat_interleave(torch.arange(ns, device=dev, dtype=torch.float32), torch.tensor(lens, device=dev))
            bp = torch.cat((bidx[:, None], pts), 1).contiguous()
            m_dyn = int(LD._dynamic_voxelize(bp, ns, rng, SY.VOXEL_01, grid, 3)["counts"][0])
            us_d = event_ms(lambda: LD._dynamic_voxelize(bp, ns, rng, SY.VOXEL_01, grid, 3), iters=20) * 1e3
            nb = 20.0 * n + 4.0 * n + m_dyn * 24.0
            entry["dynamic"] = {"us": round(us_d, 1), "GBps": round(nb / us_d / 1e3, 1), "frac": round(nb / us_d / 1e3 / PEAK_HBM_GBS, 4), "voxels": m_dyn}
            del bp, bidx
        out[label] = entry
        del pts, off, gen
    return out


def _vox_worker(args):
    """One scene through the CPU voxeliser restatement (process pool worker: the scene-parallel CPU variant of SURVEY 8d)."""
    pts, vs, rng, T, mv = args
    from oracle import lidar_oracle as LO
    g = LO.VoxelGenerator(vs, rng, 4, T, mv)
    t0 = time.perf_counter()
    g.generate(pts)
    return time.perf_counter() - t0


def cpu_voxel_baseline(scenes):
    """oracle/voxel_oracle.c on cfg-3's 8 scenes: single-threaded (what spconv's CPU generator is) and scene-parallel (one
    process per scene), median of 5 after a warm-up."""
    from lidar_vision_vqa_amd import synth as SY
    from oracle import lidar_oracle as LO
    rng = list(SY.PC_RANGE_NUSC)
    g = LO.VoxelGenerator(SY.VOXEL_01, rng, 4, 10, 160000)
    g.generate(scenes[0])
    single = []
    for _ in range(5):
        t0 = time.perf_counter()
        for s in scenes:
            g.generate(s)
        single.append(time.perf_counter() - t0)
    par = None
    try:
        import multiprocessing as mp
        ctx = mp.get_context("spawn")
        with ctx.Pool(len(scenes)) as pool:
            jobs = [(s, SY.VOXEL_01, rng, 10, 160000) for s in scenes]
            pool.map(_vox_worker, jobs)                         # warm-up: imports, the 168 MB lookup table per worker
            runs = []
            for _ in range(5):
                t0 = time.perf_counter()
                pool.map(_vox_worker, jobs)
                runs.append(time.perf_counter() - t0)
        par = float(np.median(runs))
    except Exception as err:                                    # a box without fork/spawn headroom: report the single-thread figure only
        par = None
        print(f"[bench] scene-parallel CPU voxeliser skipped: {err}", file=sys.stderr)
    n = sum(len(s) for s in scenes)
    return {"points": n, "single_thread_ms": round(float(np.median(single)) * 1e3, 2), "single_thread_mpts_per_s": round(n / np.median(single) / 1e6, 2),
            "scene_parallel_processes": len(scenes), "scene_parallel_ms": None if par is None else round(par * 1e3, 2),
            "sample": "cfg-3, 8 x 65 536 points, 0.1 m grid, T=10, 160 000 voxels: median of 5 after warm-up"}


class HeadStage:
    """BASELINE configs[3] / configs[4]: the stand-in language head behind the fused tokens.  Prefix assembly
    as validation.py:125-148 (vision prefix, LiDAR prefix, prompt, 32 answer positions), Qwen2-architecture decoder of the fused width
    (random weights: the reference's Qwen checkpoint is fetched by name), loss + the logits of the 32 answer positions."""

    def __init__(self, d, dev, precision, n_prompt=12, n_answer=32, vocab=8192, n_layers=4, seed=85):
        from lidar_vision_vqa_amd import head as HD, synth
        self.hd = HD
        self.model = HD.StandInHead(vocab, d, 4 * d, d // 64, 2, n_layers).to(dev).eval()
        synth.load_seeded(self.model, seed)
        self.model.precision = "bf16x3" if precision in ("mixed", "mixed16") else precision
        g = torch.Generator().manual_seed(seed)
        self.n_answer, self.vocab = n_answer, vocab
        self.ids = (torch.randint(4, vocab, (1, n_prompt + n_answer), generator=g)).to(dev)
        self.special = self.model.embed(torch.arange(4, device=dev).view(1, 4))[0]
        self.n_prompt = n_prompt

    def __call__(self, prefix_vision, prefix_lidar):
        B = prefix_lidar.shape[0]
        ids = self.ids.expand(B, -1)
        emb = self.model.embed(ids)
        e_prompt, e_answer = emb[:, :self.n_prompt].contiguous(), emb[:, self.n_prompt:].contiguous()
        inp, attn, labels = self.hd.assemble_prefix(prefix_vision, prefix_lidar, self.special, e_prompt, e_answer, ids[:, self.n_prompt:].contiguous())
        out = self.model(inp, attn, labels)
        return out.loss, out.logits[:, -self.n_answer:]


DUMP_BUDGET = 60 << 20      # bytes of array data one --dump-outputs writes (64 MB at most)
DUMP_WHOLE = 1 << 20        # arrays up to this size are written whole


def dump_outputs(arrays, out_dir):
    """--dump-outputs: every tensor of `arrays` as out_dir/<name>.npy, floating ones as float32, integer ones as float64 (both exact for
    what the path returns).  Arrays above DUMP_WHOLE share the rest of DUMP_BUDGET equally; each larger one keeps a sample of its rows
    (vectors along the last axis): np.random.default_rng(0).choice(n_rows, k, replace=False), sorted -- the same rows in every run that
    returns the same number of rows."""
    os.makedirs(out_dir, exist_ok=True)
    host = {k: (v.float() if v.is_floating_point() else v.double()).cpu().numpy() for k, v in arrays.items() if v is not None}
    large = sorted(k for k, a in host.items() if a.nbytes > DUMP_WHOLE)
    share = (DUMP_BUDGET - sum(a.nbytes for k, a in host.items() if k not in large)) // max(1, len(large))
    for k in large:
        a = host[k]
        rows = a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a.reshape(-1, 1)
        n = share // rows[0].nbytes
        if n < len(rows):
            rows = rows[np.sort(np.random.default_rng(0).choice(len(rows), n, replace=False))]
        host[k] = rows if a.ndim > 1 else rows[:, 0]
    for k, a in host.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", type=int, default=32, help="scenes per GPU per step")
    ap.add_argument("--precision", default="mixed", choices=list(MODES))
    ap.add_argument("--workload", default="cfg2", choices=["cfg2", "cfg4", "cfg5"], help="BASELINE configs[1] (default, the metric's own), [3] or [4]")
    ap.add_argument("--full", action="store_true", help="add the rooflines, the secondary measurements and the CPU baseline / parity check to the line")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step returned as DIR/<name>.npy (float32 / float64, <= 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and the parity check")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the secondary measurements (other modes, cross-attention rows, voxelisers, Dist-U)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    assert world == args.gpus or world == 1, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    # one rank per GPU.  With fewer devices than ranks (a rehearsal of the N > 1 path on a one-GPU box) the ranks share devices and the
    # process group falls back to gloo -- RCCL refuses two ranks on one device; such a line says so in config.parallelism
    ndev = torch.cuda.device_count()
    rehearsal = world > ndev
    local = local % max(ndev, 1)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    torch.set_grad_enabled(False)      # inference path (the reference's eval / no_grad mode)

    from lidar_vision_vqa_amd import dist as D
    from lidar_vision_vqa_amd import fusion, ops, pipeline as P, synth

    D.init_dist_if_needed("gloo" if rehearsal else None)
    wl = args.workload
    cfg = P.PipelineConfig() if wl != "cfg4" else P.PipelineConfig(n_points=120000, max_voxels_3d=160000)
    S = args.scenes
    head = None
    if wl == "cfg5":
        # token level: LiDAR tokens [S, 256, d] and image tokens [S, 576, d] resident in HBM -> VATBlock(q = LiDAR, kv = image) -> head
        pipe = None
        fuse = fusion.VATBlock(cfg.d_model, cfg.n_heads, 4 * cfg.d_model, 0.1).to(dev).eval()
        synth.load_seeded(fuse, cfg.weight_seed + 2)
        fuse.precision = args.precision
        lt = torch.from_numpy(np.stack([synth.randn((256, cfg.d_model), 5100 + 1000 * rank + i) for i in range(S)])).to(dev)
        im = torch.from_numpy(np.stack([synth.image_patches(576, cfg.d_model, 7100 + 1000 * rank + i) for i in range(S)])).to(dev)
        tokens_per_scene = 256 + 576
        workload = ("BASELINE configs[4]: 256 LiDAR tokens x 576 image tokens (d=768, 12 heads) -> VATBlock(q = LiDAR tokens, kv = image tokens) -> "
                    "prefix assembly (vision 576 | LiDAR 256 | prompt 12 | 32 answer positions: L = 880) -> stand-in Qwen2-architecture head "
                    "(d=768, 12/2 heads, 4 layers, vocab 8192) -> loss + answer logits")
    else:
        pipe = P.FusionPipeline(cfg, dev, precision=args.precision)
        # scene i of rank r: seed 1100 + 1000*r + i (SURVEY 8d cfg-4 convention)
        pts, off, patches, pts_np, patches_np = P.synthetic_batch(cfg, S, 1100 + 1000 * rank, dev)
        tokens_per_scene = cfg.n_queries
        workload = ("BASELINE configs[1]: " if wl == "cfg2" else "BASELINE configs[3] (120 000 points / scene, max_voxels 160 000, head attached): ") + cfg.describe()
    if wl in ("cfg4", "cfg5"):
        head = HeadStage(cfg.d_model, dev, args.precision)
        red = torch.zeros(2 + head.n_answer * head.vocab, dtype=torch.float32, device=dev)     # [loss sum | n_scenes | answer-logit sums]
    else:
        red = torch.zeros(cfg.d_model + 1, dtype=torch.float32, device=dev)

    def step():
        if wl == "cfg2":
            out = pipe(pts, off, patches)
            D.reduce_step(out["fused"], red)       # fused [token-sum | n_scenes] buffer, one all-reduce when world > 1
            return out
        if wl == "cfg4":
            fused = pipe(pts, off, patches)["fused"]
            loss, logits = head(patches, fused)
        else:
            fused = fuse(lt, im)
            loss, logits = head(im, fused)
        D.reduce_head_step(loss, logits, red)     # one fused buffer [loss * S | S | answer-logit sums], one all-reduce
        return dict(fused=fused, loss=loss, answer_logits=logits)

    # per-launch HIP events feed only the --full figures; when on, recording is on during warm-up too (first-use costs stay out of the
    # timed region)
    ops.EVENTS = {} if args.full else None
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ops.EVENTS = {} if args.full else None
    # a full CPython cycle collection (~30 ms with torch's module graph alive) otherwise lands inside the timed steps every
    # dozen iterations and stalls the launch stream: collect now, keep the survivors out of later scans
    gc.collect()
    gc.freeze()
    gc.disable()
    D.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps - 1):
        step()
    last = step()                   # what a caller of the timed path receives (--dump-outputs)
    torch.cuda.synchronize()
    D.barrier()
    dt = time.perf_counter() - t0
    events, ops.EVENTS = ops.EVENTS, None
    dt = D.max_over_ranks(dt, dev)
    tokens_per_step = S * tokens_per_scene
    value = world * tokens_per_step * args.steps / dt

    if rank != 0:
        gc.enable()
        D.finalize()
        return
    if args.dump_outputs:
        arrays = {**last, "reduced": red}
        # the voxel / pillar outputs are buffers of the voxelisers' capacity: rows >= scene_*_off[S] are unspecified
        for off_key, keys in (("scene_voxel_off", ("voxel_features", "voxel_coords", "voxel_num_points")),
                              ("scene_pillar_off", ("pillar_features", "pillar_coords"))):
            if off_key in arrays:
                m = int(arrays[off_key][-1])
                arrays.update({k: arrays[k][:m] for k in keys})
        dump_outputs(arrays, args.dump_outputs)
        del arrays
    del last

    prec = args.precision
    result = {
        "metric": "fused tokens/sec/GPU + cross-attn MFMA-roofline % (32k pts x 196 patches)",
        "value": round(value, 1), "unit": "fused tokens/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16", "data": "synthetic",
        "config": {"workload": workload, "scenes_per_gpu_per_step": S, "fused_tokens_per_scene": tokens_per_scene,
                   "parallelism": f"scene-parallel x{world}" + (f" (REHEARSAL: {world} ranks on {ndev} device(s), gloo)" if rehearsal else ""),
                   "precision_mode": prec + " (bf16 / fp16 MFMA tiles throughout; see parity_vs_cpu of a --full run for the error of every mode)"},
    }
    if not args.full:
        gc.enable()
        print(json.dumps(result), flush=True)
        D.finalize()
        return

    # ---- `roofline`: the cross-attention kernel at the metric's own shape (B, Nq, Nkv, d, h) = (1, 32768, 196, 768, 12), SURVEY 8d row 1 ----
    d, h = 768, 12
    blk = fusion.VATBlock(d, h, 4 * d, 0.1).to(dev).eval()
    synth.load_seeded(blk, 401)
    blk.precision = prec
    qh, kvh = torch.randn(1, 32768, d, device=dev), torch.randn(1, 196, d, device=dev)
    for _ in range(5):
        blk.cross_attention(qh, kvh)
    ops.EVENTS = {}
    for _ in range(20):
        blk.cross_attention(qh, kvh)
    torch.cuda.synchronize()
    ev_h, ops.EVENTS = ops.EVENTS, None
    flops_h = 4.0 * 32768 * d * d + 4.0 * 196 * d * d + 4.0 * 32768 * 196 * d          # SURVEY 8d F_ca: 97.5 GFLOP
    fused_route = "ca_fused" in ev_h
    if fused_route:
        ms_single = avg_ms(ev_h["ca_fused"])                    # one event pair per call: includes the event packets and an empty queue's launch gap
        ms_h = float(np.mean([event_ms(lambda: blk.cross_attention(qh, kvh), iters=20, warm=0) for _ in range(3)]))   # 20 calls back to back per event pair
        # executed MFMA FLOPs: the 196 keys run as 7 blocks of 32 (224 key slots) in both attention products and in the K|V projection
        flops_ex = 4.0 * 32768 * d * d + 4.0 * 224 * d * d + 4.0 * 32768 * 224 * d
        tr, src = profile_traffic([f"lvq_ca_fused 1x32768x196 {prec}"])
        kern = ("lvq_ca_fused = k_ca_kvproj + k_ca_fused (csrc/cross_fused.hip): LayerNorm, Q projection, softmax(Q K^T) V, out projection, bias and fp32 "
                "residual of `q + ca(ca_ln(q), kv, kv)` in one kernel, " + ("IEEE fp16" if prec != "bf16" else "bf16") + " MFMA operands (32x32x16), fp32 accumulation; "
                "HIP events on the launch stream around 20 back-to-back calls (2 launches each), mean of 3 batches; `single_call_event_ms` = one event pair per call")
    else:                                                       # bf16x3: the unfused hi + lo chain (5 launches)
        ms_h = event_ms(lambda: blk.cross_attention(qh, kvh), iters=10)
        flops_ex, tr, src, ms_single = flops_h * 3.0, None, None, None
        kern = "unfused chain (LayerNorm, Q / K|V / out projections, attention): hi + lo operands, three MFMA passes; whole sub-path"
    ach = flops_h / (ms_h * 1e-3) / 1e12
    result["roofline"] = {
        "bound": "mfma", "kernel": kern, "shape": [1, 32768, 196, d, h], "mode": prec,
        "achieved": round(ach, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_BF16_TFLOPS, 4),
        "frac_algorithmic": round(ach / PEAK_BF16_TFLOPS, 4), "frac_executed": round(flops_ex / (ms_h * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
        "flops_per_launch": flops_h, "flops_executed": flops_ex, "avg_launch_ms": round(ms_h, 4),
        "single_call_event_ms": None if ms_single is None else round(ms_single, 4), "algorithmic_bytes": 2.0 * 32768 * d * 4 + 196 * d * 4 + 4.0 * d * d * 2, "traffic": tr, "traffic_source": src,
        "hbm_floor_ms": round((2.0 * 32768 * d * 4) / (PEAK_HBM_GBS * 1e9) * 1e3, 4), "mfma_floor_ms": round(flops_h / (PEAK_BF16_TFLOPS * 1e12) * 1e3, 4)}
    del qh, kvh

    # ---- `roofline_attention`: the dominant kernel of the step (cfg2 / cfg4): VATLiDAR's cross-attention over the BEV key stream ----
    if pipe is not None:
        hh, ww = cfg.bev_hw
        per_step = cfg.n_layers + (0 if "ca_fused" in events else 1)   # attention launches per step: VATLiDAR layers (+ the fusion block's, if unfused)
        at_pairs = [p for i, p in enumerate(events.get("ca_attn", [])) if (i % per_step) < cfg.n_layers]
        at_ms = avg_ms(at_pairs)
        tc = getattr(pipe.vat_lidar, "_last_tile_counts", None)
        live_rows = int(tc[2]) if tc is not None else S * hh * ww
        if at_ms:
            dense = 4.0 * S * cfg.n_queries * (hh * ww) * d          # QK^T + PV over EVERY key (4 nq nkv d per scene)
            passes = {"bf16": 1.0, "mixed": 1.5, "mixed16": 1.0, "bf16x3": 3.0}[prec]
            pi = getattr(pipe.vat_lidar.blocks[0], "_last_pair_info", None)
            keys_streamed = S * hh * ww
            note = ""
            if pi is not None:
                pin = pi.cpu().numpy()
                keys_streamed = int(sum(int(t) * 64 if int(u) else hh * ww for t, u in pin))
                note = f"; signed pair stream: {keys_streamed} of {S * hh * ww} key slots streamed ({sum(int(u) for _, u in pin)} of {S} scenes signed)"
            streamed = 4.0 * cfg.n_queries * keys_streamed * d
            tr, src = profile_traffic([f"k_attn32 S={S} nq={cfg.n_queries} nkv={hh * ww} {prec}"])
            rate = lambda f: round(f / (at_ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4)
            result["roofline_attention"] = {
                "bound": "mfma", "kernel": f"k_attn32 (VATLiDAR.ca: {S} scenes x {cfg.n_heads} heads x {cfg.n_queries} queries over the {hh * ww}-key BEV stream, head_dim 64; "
                "32x32x16 MFMA, LDS-DMA ring, fixed softmax reference)" + note,
                # three readings, as VERDICT r2 asks: MFMA passes actually issued over the key slots actually streamed | one pass over the streamed
                # key slots (no hi + lo inflation; a dirty cell still counts twice: computed row + subtracted table row) | SURVEY 8d's dense formula
                "frac_executed": rate(streamed * passes), "frac_algorithmic_streamed": rate(streamed), "frac_dense_formula": rate(dense),
                "frac": rate(streamed * passes), "achieved": round(streamed * passes / (at_ms * 1e-3) / 1e12, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                "avg_launch_ms": round(at_ms, 4), "flops_executed": streamed * passes, "keys_streamed": keys_streamed, "keys_dense": S * hh * ww,
                "traffic": tr, "traffic_source": src}
        bk_ms = avg_ms(events.get("bev_kv", []))
        if bk_ms:
            # K|V rows out (bf16) + the table T once (fp32) + index map + the (t hi, t lo, rstd, key) rows written and read between the two launches
            nbytes = live_rows * (2 * 2 * d) + (hh * ww) * (2 * d) * 4 + S * hh * ww * 4 + 2 * live_rows * (256 + 8)
            tr, src = profile_traffic([f"k_tile_kv S={S} {prec}"])
            result["roofline_bev_kv"] = {"bound": "hbm", "kernel": "lvq_bev_tile_kv = k_conv_rows + k_kv_rows (pillar halo gather + depthwise 3x3 + GELU -> 64-channel token t -> "
                                         f"K|V = rstd (M t + m0) + T[key] for the {live_rows} dirty cells of {S * hh * ww})",
                                         "achieved": round(nbytes / (bk_ms * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                         "frac": round(nbytes / (bk_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4), "algorithmic_bytes": nbytes, "traffic": tr, "traffic_source": src,
                                         "avg_launch_ms": round(bk_ms, 4), "rows": live_rows, "rows_dense": S * hh * ww}
        g_model = pipe.vat_lidar._pe_cache.get(("stream_guard", hh, ww, dev))
        result["stream_guard"] = {"statistic_table_keys": None if g_model is None else round(g_model[1], 4), "threshold": pipe.vat_lidar.STREAM_GUARD_MAX,
                                  "tripped": getattr(pipe.vat_lidar, "_guard_tripped", None) is not None,
                                  "note": "max over (head, query) of (1 + max |score|) / sqrt(N_eff): the mixed modes keep the plain bf16 key stream only below the "
                                          "threshold (model statistic once per weights version + audits of the scenes' own key streams), else hi + lo operands"}

    mode_values = {prec: round(value, 1)}
    vscenes = None
    if not args.no_extras and world == 1 and wl == "cfg2":     # secondary measurements: single-GPU runs of the metric's own workload only
        # ---- per-stage event times of the cross-attention sub-path in the timed region ----
        result["stage_ms"] = {k: {"mean": round(avg_ms(v), 4), "max": round(max(a.elapsed_time(b) for a, b in v), 4),
                                  "min": round(min(a.elapsed_time(b) for a, b in v), 4), "launches_per_step": len(v) // args.steps}
                              for k, v in events.items()}
        # ---- the same workload in the other precision modes ----
        for mode in MODES:
            if mode == prec:
                continue
            pipe.set_precision(mode)
            n_it = max(2, args.steps // 2)
            ms = event_ms(lambda: pipe(pts, off, patches), iters=n_it, warm=2)
            mode_values[mode] = round(tokens_per_step / ms * 1e3, 1)
        pipe.set_precision(prec)
        result["value_by_mode"] = mode_values
        # ---- Dist-U scenes (SURVEY 8d cfg-2 asks for both distributions): ~1 point per voxel, worst case for the voxelisers ----
        cfg_u = P.PipelineConfig(dist="U")
        pu, ou, pau, _, _ = P.synthetic_batch(cfg_u, S, 1002, dev)
        ms_u = event_ms(lambda: pipe(pu, ou, pau), iters=max(2, args.steps // 2), warm=2)
        result["value_dist_u"] = {"value": round(tokens_per_step / ms_u * 1e3, 1), "ms_per_step": round(ms_u, 3),
                                  "note": "same pipeline and mode on Dist-U scenes (seed 1002+i); `value` is Dist-C"}
        del pu, ou, pau
        # ---- the reference's default depth: VATLiDAR(n_layers = 4); `value` is the BASELINE config's single layer (blocks 1..3 stream every
        # key through the unsigned tiled kernel: their queries depend on the scene) ----
        try:
            cfg4l = P.PipelineConfig(n_layers=4)
            p4 = P.FusionPipeline(cfg4l, dev, precision=prec)
            s4 = min(S, 8)
            b4 = P.synthetic_batch(cfg4l, s4, 1100, dev)
            ms4 = event_ms(lambda: p4(*b4[:3]), iters=3, warm=2)
            result["value_n_layers_4"] = {"value": round(s4 * cfg4l.n_queries / ms4 * 1e3, 1), "ms_per_step": round(ms4, 3), "scenes_per_step": s4,
                                          "note": "VATLiDAR with the reference's default n_layers = 4 (vat_lidar.py:67); `value` uses BASELINE's L = 1"}
            del p4, b4
        except Exception as err:                                # never let a secondary figure cost the line
            result["value_n_layers_4"] = {"error": str(err)[:200]}
        # ---- the reference's own dataflow: PointPillarScatter materialises the dense canvas, VATLiDAR.forward(bev) consumes it (round 3: the occupied
        #      cells come back out of the canvas -- lvq_bev_occupied_cells -- and the sparse key stream runs; LVQ_NO_DENSE_SPARSE=1: the dense route) ----
        try:
            sd_ = min(S, 8)
            pd = P.FusionPipeline(cfg, dev, precision=prec, dense_bev=True)
            bd = P.synthetic_batch(cfg, sd_, 1100, dev)
            msd = event_ms(lambda: pd(*bd[:3]), iters=3, warm=2)
            os.environ["LVQ_NO_DENSE_SPARSE"] = "1"
            try:
                msd0 = event_ms(lambda: pd(*bd[:3]), iters=2, warm=1)
            finally:
                del os.environ["LVQ_NO_DENSE_SPARSE"]
            result["value_dense_canvas_input"] = {"value": round(sd_ * cfg.n_queries / msd * 1e3, 1), "ms_per_step": round(msd, 3), "scenes_per_step": sd_,
                                                  "dense_route_value": round(sd_ * cfg.n_queries / msd0 * 1e3, 1), "dense_route_ms_per_step": round(msd0, 3),
                                                  "note": "same workload through the reference's call VATLiDAR.forward(bev) on a materialised [S, 64, 512, 512] canvas "
                                                          "(vat_lidar.py:187; canvas write + occupied-cell extraction included); `value` feeds the pillars directly"}
            del pd, bd
        except Exception as err:
            result["value_dense_canvas_input"] = {"error": str(err)[:200]}
        # ---- every cross-attention row of SURVEY 8d, all modes; the first row is the literal headline shape ----
        ca = cross_attention_rows(P, fusion, dev)
        result["cross_attention_rows"] = ca
        hl = ca["32k pts x 196 patches (headline)"]
        result["cross_attn_32768x196"] = {"flops": hl["flops"], **{m: hl[m] for m in MODES}}
        # ---- HBM-bound side: hard / fused-mean / dynamic voxelisers at cfg-3 ----
        hard, mean, dyn, vscenes = voxel_blocks(dev)
        result["voxelise_cfg3"] = hard
        result["voxelise_mean_cfg3"] = mean
        result["voxelise_dynamic_cfg3"] = dyn
        try:
            result["voxelise_scaling"] = voxel_scaling(dev)
        except Exception as err:
            result["voxelise_scaling"] = {"error": str(err)[:200]}

    # ---- CPU baseline: the oracle restatement on the host cores, bounded sample; parity of every timed mode against it ----
    if world == 1 and not args.no_cpu_baseline and wl == "cfg2":
        from oracle import pipeline_oracle as PO
        cores = os.cpu_count() or 1
        sd = lambda m: {k: v.detach().cpu() for k, v in m.state_dict().items()}
        sds = (sd(pipe.pillar_vfe), sd(pipe.vat_lidar), sd(pipe.fuse))
        # thread sweep on a reduced sample (1/16 of the BEV: 128 x 128 cells; same code path), 1 warm-up + 3 runs each; the full-size
        # sample then runs at the best thread count (256 threads on a 1-scene VATLiDAR oversubscribe the GEMMs)
        cfg_s = P.PipelineConfig(voxel_pillar=(0.8, 0.8, 8.0))
        sweep = {}
        for nt in sorted({t for t in (32, 64, 128, 256) if t <= cores} | {min(cores, 16)}):
            torch.set_num_threads(nt)
            PO.run(cfg_s, pts_np[:1], patches_np[:1], *sds, do_3d=False)
            ts = []
            for _ in range(3):
                t1 = time.perf_counter()
                PO.run(cfg_s, pts_np[:1], patches_np[:1], *sds, do_3d=False)
                ts.append(time.perf_counter() - t1)
            sweep[nt] = round(float(np.median(ts)), 3)
        best_t = min(sweep, key=sweep.get)
        torch.set_num_threads(best_t)
        n_par = 3 if not args.no_extras else 1                  # scenes checked for parity (the first is also the timed sample)
        refs, runs = [], []
        for i in range(n_par):
            t1 = time.perf_counter()
            refs.append(PO.run(cfg, pts_np[i:i + 1], patches_np[i:i + 1], *sds))
            runs.append(time.perf_counter() - t1)
        cpu_s = float(np.median(runs[1:])) if len(runs) > 2 else float(min(runs))      # the first run is the warm-up when there are three
        result["cpu_baseline"] = {"value": round(cfg.n_queries / cpu_s, 2), "unit": "fused tokens/s", "cores": best_t, "host_cores": cores,
                                  "kind": "port", "thread_sweep_s_on_reduced_sample": sweep,
                                  "sample": f"{n_par} scene(s) of the same workload end to end, one after the other (run times {[round(r, 1) for r in runs]} s; value = "
                                  f"median after the first, which warms up); torch fp32 on {best_t} threads = the best of the sweep {sorted(sweep)} taken on a "
                                  "1/16-size BEV; voxeliser single-threaded C like spconv's CPU generator"}
        if vscenes is not None:
            result["cpu_baseline"]["voxelise_cfg3_cpu"] = cpu_voxel_baseline(vscenes)
        parity = {}
        for mode in (MODES if not args.no_extras else (prec,)):
            pipe.set_precision(mode)
            out = pipe(pts, off, patches)
            errs = [(out["fused"][i].cpu() - refs[i]["fused"][0]).abs().max().item() for i in range(n_par)]
            parity[mode] = {"fused_max_abs_err": round(max(errs), 6), "per_scene": [round(e, 6) for e in errs], "meets_1e-3": bool(max(errs) <= TOL),
                            "value": mode_values.get(mode)}
        pipe.set_precision(prec)
        result["parity_vs_cpu"] = {"dtype": prec, "fused_max_abs_err": parity[prec]["fused_max_abs_err"], "scenes": n_par,
                                   "fused_ref_absmax": round(max(r["fused"].abs().max().item() for r in refs), 4), "tolerance": TOL,
                                   "value_meets_tolerance": parity[prec]["meets_1e-3"], "modes": parity,
                                   "note": "worst of the checked scenes (seeds 1100 + i); the cross-attention kernel of `roofline` is checked against the same "
                                           "oracle in tests/test_gpu_ca_fused.py (fp16 operands: 4.4e-4 at the headline shape)"}
    gc.enable()
    print(json.dumps(result), flush=True)
    D.finalize()


if __name__ == "__main__":
    main()
