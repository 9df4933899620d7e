#!/usr/bin/env python3
"""Debug helper for csrc/cross_fused.hip: checks the packed weight fragments and the packed K | V^T stream against numpy."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from lidar_vision_vqa_amd import _ffi as F, fusion, synth, ops

dev = torch.device("cuda:0")
torch.set_grad_enabled(False)
d, h = 768, 12
blk = fusion.VATBlock(d, h, 4 * d, 0.1).to(dev).eval()
synth.load_seeded(blk, 501)
blk.precision = "mixed"
sd = {k: v.detach().cpu().double().numpy() for k, v in blk.state_dict().items()}
blob = blk._ca_blob(True).cpu().numpy()
PKW = d * d * 2
lane = np.arange(64); n31 = lane & 31; hb = lane >> 5; j = np.arange(8)
def kidx(ks):  # [64, 8]
    return 16 * ks + 8 * (j[None, :] >> 2) + 4 * hb[:, None] + (j[None, :] & 3)
W = sd["ca.in_proj_weight"]; g = sd["ca_ln.weight"]
wq = blob[:PKW].view(np.float16).reshape(1152, 64, 8).astype(np.float64)
err = 0
for f in (0, 1, 2, 97, 500, 1151):
    hh, rem = divmod(f, 96); ks, b = rem >> 1, rem & 1
    n = 64 * hh + 32 * b + n31
    exp = (W[:d] * g[None, :])[n[:, None], kidx(ks)]
    err = max(err, np.abs(wq[f] - exp).max())
print("wq pack err", err)
wo = blob[PKW:2 * PKW].view(np.float16).reshape(1152, 64, 8).astype(np.float64)
Wo = sd["ca.out_proj.weight"]; err = 0
for f in (0, 5, 191, 192, 700, 1151):
    c, rem = divmod(f, 192); ks, nb = rem >> 2, rem & 3
    n = 128 * c + 32 * nb + n31
    err = max(err, np.abs(wo[f] - Wo[n[:, None], kidx(ks)]).max())
print("wo pack err", err)
tabs = blob[4 * PKW:4 * PKW + 3 * d * 4].view(np.float32).reshape(3, d).astype(np.float64)
qs = 1.4426950408889634 / 8
bq = (sd["ca.in_proj_bias"][:d] + W[:d] @ sd["ca_ln.bias"]) * qs
print("bq err", np.abs(tabs[0] - bq).max(), "sn err", np.abs(tabs[1] - (W[:d] * g[None]).astype(np.float16).astype(np.float64).sum(1)).max(),
      "bo err", np.abs(tabs[2] - sd["ca.out_proj.bias"]).max())

B, nq, nkv = 1, 128, 196
q, kv = synth.randn((B, nq, d), 502), synth.randn((B, nkv, d), 503)
out = blk.cross_attention(torch.from_numpy(q).to(dev), torch.from_numpy(kv).to(dev))
torch.cuda.synchronize()
ws = F._WORKSPACES[(0, "ca_fused", None)].cpu().numpy()
KC, CF = 7, 64
fr = ws[:B * h * CF * 1024].view(np.float16).reshape(B, h, CF, 64, 8).astype(np.float64)
K = kv[0].astype(np.float64) @ W[d:2 * d].T + sd["ca.in_proj_bias"][d:2 * d]
V = kv[0].astype(np.float64) @ W[2 * d:].T + sd["ca.in_proj_bias"][2 * d:]
Kp = np.zeros((224, d)); Kp[:nkv] = K; Kp[nkv:] = sd["ca.in_proj_bias"][d:2 * d]
Vp = np.zeros((224, d)); Vp[:nkv] = V; Vp[nkv:] = sd["ca.in_proj_bias"][2 * d:]
ek = ev = 0
for hh in (0, 5, 11):
    for kb in range(KC):
        for s in range(4):
            blkd, sp = s >> 1, s & 1
            key = 32 * kb + n31
            dh = 64 * hh + 32 * blkd + 16 * sp + 8 * (j[None, :] >> 2) + 4 * hb[:, None] + (j[None, :] & 3)
            ek = max(ek, np.abs(fr[0, hh, kb * 4 + s] - Kp[key[:, None], dh]).max())
        for t in range(2):
            for b in range(2):
                dh = 64 * hh + 32 * b + n31
                key = 32 * kb + 16 * t + 8 * (j[None, :] >> 2) + 4 * hb[:, None] + (j[None, :] & 3)
                ev = max(ev, np.abs(fr[0, hh, 4 * KC + kb * 4 + 2 * t + b] - Vp[key, dh[:, None]]).max())
print("K frag err", ek, "V frag err", ev, " (fp16 rounding ~1e-3 expected)")
from oracle import vat_oracle as VO
sdt = {k: v.detach().cpu() for k, v in blk.state_dict().items()}
qt, kvt = torch.from_numpy(q), torch.from_numpy(kv)
ref = qt + VO.mha(VO.layer_norm(qt, sdt["ca_ln.weight"], sdt["ca_ln.bias"]), kvt, sdt, "ca.", h)
e = (out.cpu() - ref).abs()
print("out err max", e.max().item(), "per-row max (first 8 rows)", e[0, :8].max(-1).values.tolist())
print("err by column block of 128:", [round(e[0, :, c * 128:(c + 1) * 128].max().item(), 4) for c in range(6)])
print("err by wave:", [round(e[0, w * 32:(w + 1) * 32].max().item(), 4) for w in range(4)])

# ---- which wrong formula matches the GPU output best? ----
def emul(var):
    x = q[0].astype(np.float64); kvd = kv[0].astype(np.float64)
    g = sd["ca_ln.weight"]; b = sd["ca_ln.bias"]
    mu = x.mean(-1, keepdims=True); v = ((x - mu) ** 2).mean(-1, keepdims=True); rstd = 1 / np.sqrt(v + 1e-5)
    Wq = W[:d] * g[None]; bqq = sd["ca.in_proj_bias"][:d] + W[:d] @ b
    c = x[:, :64].mean(-1, keepdims=True)
    dd = x - c; mud = dd.mean(-1, keepdims=True)
    acc = dd @ Wq.T; sn = Wq.sum(1)
    if var == "nomean": Q = acc * rstd + bqq
    elif var == "signmean": Q = (acc + mud * sn[None]) * rstd + bqq
    elif var == "nobias": Q = (acc - mud * sn[None]) * rstd
    else: Q = (acc - mud * sn[None]) * rstd + bqq
    Q = Q / 8
    out = np.zeros_like(x)
    O = np.zeros_like(x)
    nk = 224 if var == "nomask" else nkv
    Kx, Vx = (Kp, Vp) if var == "nomask" else (K, V)
    for hh in range(h):
        sl = slice(64 * hh, 64 * hh + 64)
        S = Q[:, sl] @ Kx[:nk, sl].T
        P = np.exp(S - S.max(-1, keepdims=True))
        if var == "halfsum": P = P / (P.sum(-1, keepdims=True) * 0.5)
        else: P = P / P.sum(-1, keepdims=True)
        O[:, sl] = P @ Vx[:nk, sl]
    res = O @ Wo.T + (0 if var == "nobo" else sd["ca.out_proj.bias"])
    return x + res
g_out = out.cpu().numpy()[0].astype(np.float64)
for var in ("exact", "nomean", "signmean", "nobias", "nomask", "halfsum", "nobo"):
    print(var, np.abs(emul(var) - g_out).max())
