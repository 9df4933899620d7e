#!/usr/bin/env python3
"""Timing of the CLIP-L tower (clip_tower.build_clip_l, seeded weights) on SAM-shaped features [B, 1024, 16, 16] and of the whole
deepencoder.DeepEncoderRuntime.encode_pixels (SAM ViT-B -> CLIP-L -> projector, 1024 x 1024 images), for B = 1 and 6 in both operand
forms.  Report only: this path has not been measured before, there is no reference number on this hardware and no target.

  forward_ms    device events around `iters` back-to-back forwards, divided by iters; `reps` such windows after a warm-up of every shape:
                the median, with the smallest and largest window as the spread
  kernels       per kind of launch of the CLIP tower and the join (gemm, attention, layernorm, embed): device events around every tagged
                call (ops.EVENTS), in a run of their own; `forward_minus_tagged` is the forward less their sum -- torch copies,
                lvq_cast_bf16, and in encode_pixels the whole SAM tower (tools/bench_vision_tower.py splits that one).  An event pair
                around a launch of a few microseconds also times the gap to the next launch, so for the tower alone (about 170 short
                launches) the tagged sum comes out ABOVE the back-to-back forward and the difference is negative: read the split as
                shares of the tagged sum, not as absolute times
  embed_ab      lvq_clip_embed (hidden + the token-major operand) against what it replaces -- transpose, cat, position add by torch,
                lvq_layernorm, and a second permute + lvq_cast_bf16 for the operand -- in alternation
  fc1_ab        fc1 with LVQ_GEMM_QUICK_GELU against fc1 to fp32 + a torch elementwise x sigmoid(1.702 x) + lvq_cast_bf16, in alternation
  depth24_error the 24-layer tower against an fp64 torch replay (tests/clip_tower_cases.py: vit) on the same seeded weights, both modes:
                max |out - ref| / max(1, max|ref|) (a report; tests/test_gpu_deepencoder_full.py holds depth 24 to its bounds)

    python tools/bench_deepencoder.py [--iters 10] [--reps 5] [--out profiles/deepencoder.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import clip_tower_cases as CC  # noqa: E402
from lidar_vision_vqa_amd import clip_tower as CT, deepencoder as DE, fusion, ops as O, synth, vision_tower as VT  # noqa: E402

MODES = ("bf16x3", "bf16")
KINDS = {"clip_gemm": "gemm", "clip_attn": "attention", "clip_ln": "layernorm", "clip_embed": "embed"}


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def windows(fn, iters, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = [window(fn, iters) for _ in range(reps)]
    return float(np.median(out)), float(min(out)), float(max(out))


def stat(v):
    return [round(float(np.median(v)), 4), round(float(min(v)), 4), round(float(max(v)), 4)]


def alternate(a, b, iters, reps):
    for _ in range(2):
        a(), b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(max(5, reps)):
        ta.append(window(a, iters))
        tb.append(window(b, iters))
    return stat(ta), stat(tb)


def split_by_kind(forward, iters):
    for _ in range(2):
        forward()
    torch.cuda.synchronize()
    O.EVENTS = {}
    try:
        for _ in range(iters):
            forward()
        torch.cuda.synchronize()
        rec = O.EVENTS
    finally:
        O.EVENTS = None
    return {KINDS[tag]: {"launches": len(ev) // iters, "ms": round(sum(s.elapsed_time(e) for s, e in ev) / iters, 4)} for tag, ev in rec.items()
            if tag in KINDS}


def measure(what, forward, shape, mode, iters, reps):
    out = forward()
    med, lo, hi = windows(forward, iters, reps)
    kinds = split_by_kind(forward, iters)
    kinds["forward_minus_tagged"] = {"launches": None, "ms": round(med - sum(v["ms"] for v in kinds.values()), 4)}
    r = {"what": what, "mode": mode, "in": list(shape), "out": list(out.shape), "forward_ms": round(med, 3), "forward_ms_min": round(lo, 3),
         "forward_ms_max": round(hi, 3), "kernels": kinds}
    if "attention" in kinds:
        r["attention_share_of_tagged_launches"] = round(kinds["attention"]["ms"] / sum(v["ms"] for k, v in kinds.items() if k != "forward_minus_tagged"), 4)
    print(f"{what} {list(shape)} {mode}: {med:.3f} ms [{lo:.3f}, {hi:.3f}]  " + "  ".join(f"{k} {v['ms']:.3f}" for k, v in kinds.items()), flush=True)
    return r


def embed_ab(clip, batch, split, iters, reps, dev):
    feat4 = torch.from_numpy(synth.randn((batch, 1024, 16, 16), 7000 + batch)).to(dev)
    emb, ln = clip.embeddings, clip.pre_layrnorm
    cls, pos = emb.class_embedding.detach(), emb._pos_table(257)
    g, b = ln.weight.detach(), ln.bias.detach()

    def new():
        return O.clip_embed(feat4.flatten(2), cls, pos, g, b, ln.eps, want_tok=True, split=split)

    def parent():
        tok = feat4.flatten(2).transpose(1, 2)
        rows = (torch.cat((cls.expand(batch, 1, -1), tok), 1) + pos).reshape(-1, 1024)
        hidden, _ = O.layernorm(rows, g, b, ln.eps, split, want_f32=True, want_bf=False)
        return hidden, O.cast(feat4.flatten(2).permute(0, 2, 1).contiguous().view(-1, 1024), split)

    (h1, t1), (h0, t0) = new(), parent()
    agree = float((h1 - h0).abs().max())
    assert torch.equal(t1[0], t0[0])
    tn, tp = alternate(new, parent, iters, reps)
    return {"batch": batch, "mode": "bf16x3" if split else "bf16", "lvq_clip_embed_ms": tn, "torch_rows_layernorm_cast_ms": tp,
            "max_abs_difference_of_hidden": agree}


def fc1_ab(clip, batch, split, iters, reps, dev):
    mlp = clip.transformer.layers[0].mlp
    h = O.cast(torch.from_numpy(synth.randn((batch * 257, 1024), 7100 + batch)).to(dev), split)
    w, bias = CT._operand(mlp.fc1, "weight", split), mlp.fc1.bias.detach()

    def new():
        return O.linear(h, w, bias, quick_gelu=True, out_bf=True)[1]

    def parent():
        y, _ = O.linear(h, w, bias, out_f32=True)
        return O.cast(y * torch.sigmoid(1.702 * y), split)

    a, b = new(), parent()
    agree = float((a[0].float() - b[0].float()).abs().max())
    tn, tp = alternate(new, parent, iters, reps)
    return {"rows": batch * 257, "mode": "bf16x3" if split else "bf16", "flag_ms": tn, "gemm_torch_elementwise_cast_ms": tp,
            "max_abs_difference_of_bf16_outputs": agree}


def depth24_error(clip, sd, dev):
    x = synth.randn((1, 3, 224, 224), 7200)
    pe = synth.randn((1, 1024, 16, 16), 7201)
    with torch.no_grad():
        ref = CC.vit(sd, dict(CC.WIDE, num_layers=24), x, pe).numpy()
    out = {}
    for mode in MODES:
        clip.precision = mode
        with torch.no_grad():
            got = clip(torch.from_numpy(x).to(dev), torch.from_numpy(pe).to(dev)).cpu().numpy()
        out[mode] = float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))
    out["max_abs_ref"] = float(np.abs(ref).max())
    out["note"] = "24 layers, seeded weights (tests/clip_tower_cases.py scales), one image"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deepencoder.py needs an MI355X: there is no CPU timing of this path")
    dev = torch.device("cuda:0")
    res = {"what": "CLIP-L tower and DeepEncoderRuntime.encode_pixels on liblvq_hip.so; first measurement of this path, no reference number exists",
           "device": torch.cuda.get_device_name(0), "iters": a.iters, "reps": a.reps,
           "ms_fields": "median over reps windows; *_min / *_max or [median, min, max] give the spread", "forward": [], "embed_ab": [], "fc1_ab": []}
    sd = CC.state(dict(CC.WIDE, num_layers=24), 81)
    clip = CT.build_clip_l()
    clip.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    clip = clip.to(dev).eval().requires_grad_(False)
    for batch in (1, 6):
        x = torch.zeros((batch, 3, 224, 224), device=dev)
        pe = torch.from_numpy(synth.randn((batch, 1024, 16, 16), 7300 + batch)).to(dev)
        for mode in MODES:
            clip.precision = mode

            def forward():
                with torch.no_grad():
                    return clip(x, pe)
            res["forward"].append(measure("clip_l", forward, pe.shape, mode, a.iters, a.reps))
    for batch in (1, 6):
        for split in (True, False):
            res["embed_ab"].append(embed_ab(clip, batch, split, 10 * a.iters, a.reps, dev))
            res["fc1_ab"].append(fc1_ab(clip, batch, split, 10 * a.iters, a.reps, dev))
            print(json.dumps(res["embed_ab"][-1]), json.dumps(res["fc1_ab"][-1]), flush=True)
    res["depth24_error"] = depth24_error(clip, sd, dev)
    print("depth 24:", json.dumps(res["depth24_error"]), flush=True)
    rt = DE.DeepEncoderRuntime.from_modules(synth.load_seeded(VT.build_sam_vit_b(), 9), clip, synth.load_seeded(fusion.MlpProjectorLinear(2048, 2048), 10),
                                            device=dev)
    for batch in (1, 6):
        x = torch.from_numpy(synth.randn((batch, 3, 1024, 1024), 7400 + batch)).to(dev)
        for mode in MODES:
            rt.precision = mode
            res["forward"].append(measure("encode_pixels", lambda: rt.encode_pixels(x), x.shape, mode, a.iters, a.reps))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
