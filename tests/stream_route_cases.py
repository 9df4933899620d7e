"""Host-only inputs and fp64 references for the three long-stream entry points of csrc/attention.hip that VATLiDAR's cross-attention
runs through (lvq_attention_bf16_tiled, lvq_attention_bf16_tiled_signed, lvq_attention_bf16_stream_totals).  torch on the CPU only: no
GPU import, nothing a kernel produced.  tests/test_stream_route_cases.py holds the conditions under which the inputs can tell a wrong
kernel from a right one, tests/test_gpu_stream_routes.py runs the kernels.

Inputs -- a PEAKED stream with probes.  All table rows (64 n_tiles) and all computed rows are N(0, 1) rounded to bf16 (K to fp16 in the
mixed16 form); V is independent of K.  ONE K|V buffer: [table rows | `gap` unused rows holding PAD_VALUE | computed rows].  The queries
are shared by the batch elements (the signed stream needs that).  Query i of head h has three probe rows and is the minimum-norm vector
whose scaled score is 10 nats on exactly those (q = Kp^T (Kp Kp^T)^-1 (10 / scale) 1, on the K values the kernel will see):

    A  the table row of a STRUCTURAL slot (first / last slot of the stream, the tile 0 | 1 edge, both sides of every 8-tile row-word
       window boundary and of every KV-split boundary sp * ceil(n_tiles / nsplit) of the split counts used, the last tile).  Structural
       slots are clean in every batch element; query (h, i) takes slot number (h nq + i) mod len(list).
    C  a computed row at a cell that is dirty in every batch element with dirty cells (the same row in all of them: any numbering of
       the computed rows is legal)
    S  the table row of another such cell: present in the totals and in a clean batch element, and what a signed batch has to SUBTRACT
  There are 16 C cells and 16 S cells; of the 256 (C, S) pairs a query takes the one that gives the shortest q, because |q|^2 is the
  variance of its scores on all other keys: nearly collinear probe rows would hand the mass back to the diffuse background.

A batch element ("scene") is given by its number of dirty cells: 0 = clean (probes A, S), >= 32 = the 16 C cells, the 16 S cells and
random further cells (probes A, C; S must be subtracted by the signed stream).  With `trip`, query 0 of head 0 instead scores 16 nats on
ONE S row: the signed row sum of that row is far below 1/16 of the table's, which flags (batch, head 0) for the predicated re-run.

Reference -- fp64, operands as the kernel sees them (attention.hip: "Q^T fragments, pre-multiplied by scale * log2(e)"), with
c = fp32(scale) * 1.4426950408889634f and x = (hi + lo) * c in fp32:
    plain   bf16(hi * c)                           split   hi' = bf16(x), lo' = bf16(x - hi'): hi' + lo'
    f16     fp16(x)                                f16x2   fp16(x) + fp16(x - fp16(x))      (the totals with k_fp16 = 2)
scores s = q' . k exactly, p = 2^(s - max), o = sum p v / sum p over each batch element's row_src rows -- for the tiled and the signed
call alike.

Bounds -- per element, from fp64 quantities only (w = p / sum p):
    tiled    |o - ref| <= 2^-8 sum_j w_j |v_j| + R.  P is rounded to bf16 before P V: between 2^-9 (top of a binade) and 2^-8 (bottom)
             relative per weight, so 2^-8 sum w |v| covers every P (twice the error of weights near the top of their binade).
             R = 2^-9 |ref| for one bf16 output, 2^-16 for hi + lo outputs.
    signed   sum w |v| -> (A_tot + A_sub + A_new) / l_final, A = unnormalised sum p |v| over all table keys, the subtracted table keys
             and the computed rows (each sum carries its own P rounding once its softmax reference differs), plus
             2^-20 (l_tot + l_sub + l_new) / l_final |ref| for the fp32 cancellation.
    totals   O / l as tiled (R = 0: fp32 output); m + log2 l against log2 sum_j 2^(s_j) within nkv 2^-23 (fp32 summation, doubled).
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch

PAD_VALUE = 77.0
DH = 64
SCALE = 0.125
NATS = 10.0
TRIP_NATS = 16.0
N_C = 16                    # cells whose computed row is a probe
N_S = 16                    # cells whose table row is a probe and that every dirty scene replaces
QFORMS = ("plain", "split", "f16", "f16x2")


@dataclass(frozen=True)
class Spec:
    nq: int
    n_tiles: int
    scenes: tuple            # dirty cells per batch element: 0, or >= N_C + N_S
    splits: tuple = (1, 3, 8)
    H: int = 2
    gap: int = 0             # unused rows between the table and the computed rows (row_base = 64 n_tiles + gap)
    k16: bool = False        # K as IEEE fp16 (mixed16)
    trip: bool = False
    seed: int = 1

    @property
    def B(self):
        return len(self.scenes)

    @property
    def nkv(self):
        return 64 * self.n_tiles

    @property
    def row_base(self):
        return self.nkv + self.gap

    def pair_tiles(self, b):
        return (self.scenes[b] + 31) // 32

    def signed(self, b):
        """lvq_bev_scene_pairs: a batch element streams its pair list when that is shorter than its full tile list."""
        return self.pair_tiles(b) < self.n_tiles


def structural_slots(n_tiles, splits):
    nkv = 64 * n_tiles
    s = {0, nkv - 1, 63, 64}
    for t in range(8, n_tiles, 8):                       # row-word windows of 8 tiles (from the start of the stream)
        s |= {64 * t - 1, 64 * t}
    for ns in splits:
        tps = (n_tiles + ns - 1) // ns
        for sp in range(1, ns):
            t0 = sp * tps
            if t0 < n_tiles:
                s |= {64 * t0 - 1, 64 * t0}
                for t in range(t0 + 8, n_tiles, 8):      # ... and from the start of every split
                    s |= {64 * t - 1, 64 * t}
    if n_tiles % 8:
        s |= {64 * (n_tiles - 1), 64 * (n_tiles - 1) + 31, nkv - 2}
    return sorted(s)


@dataclass
class Inputs:
    spec: Spec
    k: torch.Tensor          # [rows, d] fp32, exactly representable in bf16 (fp16 with k16)
    v: torch.Tensor          # [rows, d] fp32, bf16 values
    q: torch.Tensor          # [nq, d] fp32; the kernels get hi = bf16(q), lo = bf16(q - hi)
    row_src: torch.Tensor    # [B, nkv] int32
    slots: list              # structural slots
    probe_a: torch.Tensor    # [H, nq] slot
    probe_c: torch.Tensor    # [H, nq] slot (its computed row is row_base + index in c_cells)
    probe_s: torch.Tensor    # [H, nq] slot
    c_cells: torch.Tensor
    s_cells: torch.Tensor

    @property
    def q_hi(self):
        return self.q.to(torch.bfloat16)

    @property
    def q_lo(self):
        return (self.q - self.q_hi.float()).to(torch.bfloat16)

    def pair_lists(self, cap_tiles, fill_row=0):
        """What lvq_bev_scene_pairs documents (include/lvq.h), built on the host: tile j of a batch element = its dirty rows 32 j .. + 31
        in slot order (keys 0..31) | the table rows of the same cells (keys 32..63); padding = table row 0 in both halves; a list that
        would not be shorter than the stream is not written (pair_info = 0, 0).  Everything else holds `fill_row`."""
        sp = self.spec
        ps = torch.full((sp.B, cap_tiles, 64), fill_row, dtype=torch.int32)
        pi = torch.zeros((sp.B, 2), dtype=torch.int32)
        for b in range(sp.B):
            if not sp.signed(b):
                continue
            e = torch.nonzero(self.row_src[b] >= sp.row_base).view(-1)
            n_pt = sp.pair_tiles(b)
            rows = torch.zeros(32 * n_pt, dtype=torch.int32)
            cells = torch.zeros(32 * n_pt, dtype=torch.int32)
            rows[:len(e)] = self.row_src[b, e]
            cells[:len(e)] = e.to(torch.int32)
            ps[b, :n_pt, :32] = rows.view(n_pt, 32)
            ps[b, :n_pt, 32:] = cells.view(n_pt, 32)
            pi[b, 0], pi[b, 1] = n_pt, 1
        return ps, pi


@functools.lru_cache(maxsize=None)
def build(spec: Spec) -> Inputs:
    g = torch.Generator().manual_seed(1000 + spec.seed)
    H, nq, nkv, d = spec.H, spec.nq, spec.nkv, spec.H * DH
    slots = structural_slots(spec.n_tiles, spec.splits)
    assert len(slots) <= H * nq
    free = torch.ones(nkv, dtype=torch.bool)
    free[slots] = False
    perm = torch.randperm(nkv, generator=g)
    perm = perm[free[perm]]
    c_cells, s_cells, pool = perm[:N_C], perm[N_C:N_C + N_S], perm[N_C + N_S:]
    # rows: table | gap | the N_C shared probe rows | every dirty scene's own rows | 7 rows nobody uses
    own = [max(0, n - N_C) for n in spec.scenes]
    assert all(n == 0 or n >= N_C + N_S for n in spec.scenes) and max(own) - N_S <= len(pool)
    rows = spec.row_base + N_C + sum(own) + 7
    k = torch.randn(rows, d, generator=g)
    v = torch.randn(rows, d, generator=g).to(torch.bfloat16).float()
    k = k.half().float() if spec.k16 else k.to(torch.bfloat16).float()
    k[nkv:spec.row_base] = PAD_VALUE
    v[nkv:spec.row_base] = PAD_VALUE
    row_src = torch.arange(nkv, dtype=torch.int32).repeat(spec.B, 1)
    nxt = spec.row_base + N_C
    for b, n in enumerate(spec.scenes):
        if n == 0:
            continue
        row_src[b, c_cells] = spec.row_base + torch.arange(N_C, dtype=torch.int32)
        mine = torch.cat((s_cells, pool[torch.randperm(len(pool), generator=g)[:n - N_C - N_S]]))
        num = torch.randperm(len(mine), generator=g).to(torch.int32)            # any numbering of the computed rows is legal
        row_src[b, mine] = nxt + num
        nxt += len(mine)
    # probes and queries
    # A is fixed by the walk over the structural slots.  Of the N_C x N_S (C, S) pairs each query takes the one that gives the shortest
    # q: |q|^2 is the variance of its scores on the other keys, i.e. what decides how much mass the diffuse background keeps
    idx = torch.arange(H * nq).view(H, nq)
    ia = idx % len(slots)
    probe_a = torch.tensor(slots)[ia]
    ic, i_s = torch.empty_like(idx), torch.empty_like(idx)
    q = torch.empty(nq, d)
    cc, ss = torch.arange(N_C).repeat_interleave(N_S), torch.arange(N_S).repeat(N_C)                     # the candidate pairs
    rhs = torch.full((nq, N_C * N_S, 3, 1), NATS / SCALE, dtype=torch.float64)
    for h in range(H):
        c = slice(DH * h, DH * h + DH)
        kd = k[:, c].double()
        kp = torch.stack((kd[probe_a[h]].unsqueeze(1).expand(nq, N_C * N_S, DH), kd[spec.row_base + cc].expand(nq, -1, -1),
                          kd[s_cells[ss]].expand(nq, -1, -1)), 2)                                        # [nq, pairs, 3, 64]
        y = torch.linalg.solve(kp @ kp.transpose(2, 3), rhs)
        best = (rhs * y).sum((2, 3)).argmin(1)                                                           # |q|^2 = rhs^T G^-1 rhs
        ic[h], i_s[h] = cc[best], ss[best]
        ar = torch.arange(nq)
        q[:, c] = (kp[ar, best].transpose(1, 2) @ y[ar, best]).squeeze(-1).float()
    probe_c, probe_s = c_cells[ic], s_cells[i_s]
    if spec.trip:
        ks = k[probe_s[0, 0], :DH].double()
        q[0, :DH] = ((TRIP_NATS / SCALE) * ks / (ks @ ks)).float()
    hi = q.to(torch.bfloat16).float()
    q = hi + (q - hi).to(torch.bfloat16).float()             # exactly hi + lo
    return Inputs(spec, k, v, q, row_src, slots, probe_a, probe_c, probe_s, c_cells, s_cells)


def scaled_query(inp: Inputs, qform: str) -> torch.Tensor:
    """The query the MFMAs see, [nq, d] fp64, in log2 units."""
    c = torch.tensor(float(np.float32(SCALE) * np.float32(1.4426950408889634)), dtype=torch.float32)
    hi, lo = inp.q_hi.float(), inp.q_lo.float()
    if qform == "plain":
        return (hi * c).to(torch.bfloat16).double()
    x = (hi + lo) * c
    if qform == "split":
        h2 = x.to(torch.bfloat16).float()
        return h2.double() + (x - h2).to(torch.bfloat16).double()
    h2 = x.half().float()
    if qform == "f16":
        return h2.double()
    assert qform == "f16x2"
    return h2.double() + (x - h2).half().double()


@functools.lru_cache(maxsize=4)
def _scores(spec: Spec, qform: str) -> torch.Tensor:
    """[H, nq, rows]: every query against every row of the buffer (the gap rows included: nothing may gather them)."""
    inp = build(spec)
    q = scaled_query(inp, qform)
    k = inp.k.double()
    return torch.stack([q[:, DH * h:DH * h + DH] @ k[:, DH * h:DH * h + DH].t() for h in range(spec.H)])


def _heads(x, H):
    """[n, H * 64] -> [H, n, 64]"""
    return x.view(x.shape[0], H, DH).transpose(0, 1)


def _flat(o):
    """[H, nq, 64] -> [nq, H * 64]"""
    return o.transpose(0, 1).reshape(o.shape[1], -1)


@dataclass
class Ref:
    o: torch.Tensor          # [nq, d]
    absv: torch.Tensor       # [nq, d]  sum w |v| (tiled) or (A_tot + A_sub + A_new) / l_final (signed)
    cancel: torch.Tensor     # [nq, d]  2^-20 (l_tot + l_sub + l_new) / l_final |ref| (signed), 0 otherwise
    lse2: torch.Tensor       # [H, nq]  log2 sum 2^s
    ratio: torch.Tensor      # [H, nq]  l_final / l_tot (signed) or None

    def bound(self, out_lo: bool, r=None):
        rr = (2.0 ** -16 if out_lo else 2.0 ** -9 * self.o.abs()) if r is None else r
        return 2.0 ** -8 * self.absv + self.cancel + rr


def _softmax_sums(s, v, shift):
    """s [H, nq, n], v [n, d], shift [H, nq] -> l [H, nq], sum p v, sum p |v| ([H, nq, 64]) with p = 2^(s - shift)."""
    p = torch.exp2(s - shift.unsqueeze(-1))
    vh = _heads(v.double(), s.shape[0])
    return p.sum(-1), p @ vh, p @ vh.abs()


@functools.lru_cache(maxsize=32)
def reference(spec: Spec, qform: str, b: int, signed: bool = False) -> Ref:
    """Batch element b: the full softmax over its row_src rows; with `signed` the bound of the signed stream."""
    inp = build(spec)
    S = _scores(spec, qform)
    src = inp.row_src[b].long()
    s = S[:, :, src]
    m = s.max(-1).values
    l, pv, pa = _softmax_sums(s, inp.v[src], m)
    o = pv / l.unsqueeze(-1)
    lse2 = m + torch.log2(l)
    if not signed:
        return Ref(_flat(o), _flat(pa / l.unsqueeze(-1)), torch.zeros_like(_flat(o)), lse2, None)
    nkv = spec.nkv
    dirty = torch.nonzero(src >= spec.row_base).view(-1)
    s_tab = S[:, :, :nkv]
    M = torch.maximum(m, s_tab.max(-1).values)
    l_tot, _, a_tot = _softmax_sums(s_tab, inp.v[:nkv], M)
    l_sub, _, a_sub = _softmax_sums(s_tab[:, :, dirty], inp.v[dirty], M)
    l_new, _, a_new = _softmax_sums(s[:, :, dirty], inp.v[src[dirty]], M)
    l_fin = l * torch.exp2(m - M)
    absv = (a_tot + a_sub + a_new) / l_fin.unsqueeze(-1)
    cancel = 2.0 ** -20 * ((l_tot + l_sub + l_new) / l_fin).unsqueeze(-1) * o.abs()
    return Ref(_flat(o), _flat(absv), _flat(cancel), lse2, l_fin / l_tot)


@functools.lru_cache(maxsize=8)
def totals_reference(spec: Spec, qform: str) -> Ref:
    """The per-model totals: the softmax over the table rows 0 .. nkv - 1 alone, as o = O / l and lse2 = m + log2 l."""
    inp = build(spec)
    s = _scores(spec, qform)[:, :, :spec.nkv]
    m = s.max(-1).values
    l, pv, pa = _softmax_sums(s, inp.v[:spec.nkv], m)
    o = pv / l.unsqueeze(-1)
    return Ref(_flat(o), _flat(pa / l.unsqueeze(-1)), torch.zeros_like(_flat(o)), m + torch.log2(l), None)


# ---- what the CPU test asks of the inputs -------------------------------------------------------------------------------------
def probe_effects(spec: Spec, qform: str, b: int, signed: bool):
    """For batch element b -> list of (name, mass [H, nq], moved [H, nq]): the softmax mass each probe holds in the reference and the
    largest |change| over the 64 outputs of its row when a kernel loses that key (A, C / S present in the stream), fails to subtract
    the S table row, or fails to add the C row (signed)."""
    inp = build(spec)
    S = _scores(spec, qform)
    ref = reference(spec, qform, b, signed)
    o = ref.o.view(spec.nq, spec.H, DH).transpose(0, 1)                       # [H, nq, 64]
    src = inp.row_src[b].long()
    vh = _heads(inp.v.double(), spec.H)                                       # [H, rows, 64]
    hh = torch.arange(spec.H).view(-1, 1)
    ii = torch.arange(spec.nq).view(1, -1)
    out = []

    def effect(rows, sign):
        """weight of buffer row rows[h, i] relative to the row sum; lost (sign -1) or wrongly present (sign +1)"""
        w = torch.exp2(S[hh, ii, rows] - ref.lse2)
        delta = (w / (1.0 + sign * w)).unsqueeze(-1) * (vh[hh, rows] - o)
        return w, delta.abs().max(-1).values

    dirty_scene = spec.scenes[b] > 0
    out.append(("A",) + effect(src[inp.probe_a], -1))
    if dirty_scene:
        out.append(("C",) + effect(src[inp.probe_c], -1))                     # = "not adding the computed-row probe"
        if signed:
            w, moved = effect(inp.probe_s, +1)                                # the table row of a dirty cell, left in
            out.append(("S not subtracted", None, moved))
    else:
        out.append(("S",) + effect(src[inp.probe_s], -1))
    return out


def emulate_bf16_p(spec: Spec, qform: str, b: int, signed: bool, out_lo: bool):
    """The reference with P rounded to bf16 before P V (the row sum from the unrounded P, as the kernel forms it) and the output rounded:
    what a correct kernel may return.  Signed: the three sums (totals, subtracted, added) round their P at three different softmax
    references, as after a rescale."""
    inp = build(spec)
    S = _scores(spec, qform)
    src = inp.row_src[b].long()
    H = spec.H
    bf = lambda x: x.float().to(torch.bfloat16).double()

    def sums(s, v, shift):
        p = torch.exp2(s - shift.unsqueeze(-1))
        return p.sum(-1), bf(p) @ _heads(v.double(), H)

    s = S[:, :, src]
    m = s.max(-1).values
    if not signed:
        l, pv = sums(s, inp.v[src], m - 3.0)
        o = pv / l.unsqueeze(-1)
    else:
        dirty = torch.nonzero(src >= spec.row_base).view(-1)
        s_tab = S[:, :, :spec.nkv]
        M = torch.maximum(m, s_tab.max(-1).values)
        shifts = (M - 0.3, M - 1.7, M - 2.45)
        lt, ot = sums(s_tab, inp.v[:spec.nkv], shifts[0])
        ls, os_ = sums(s_tab[:, :, dirty], inp.v[dirty], shifts[1])
        ln, on = sums(s[:, :, dirty], inp.v[src[dirty]], shifts[2])
        w = [torch.exp2(x - M) for x in shifts]
        l = lt * w[0] - ls * w[1] + ln * w[2]
        o = (ot * w[0].unsqueeze(-1) - os_ * w[1].unsqueeze(-1) + on * w[2].unsqueeze(-1)) / l.unsqueeze(-1)
    o = _flat(o).float()
    hi = o.to(torch.bfloat16)
    return hi.double() + ((o - hi.float()).to(torch.bfloat16).double() if out_lo else 0.0)


# ---- the cases of tests/test_gpu_stream_routes.py (n_tiles in {64, 67, 72}, H = 2, B <= 3) ----------------------------------------
# `splits` lists every KV split count the GPU tests run the spec with (plan_attn's own choice is n_tiles / 8 = 8 or 9 at these sizes).
SPECS = {
    "w6_176": Spec(176, 64, (600, 0, 33), seed=1),                            # 6 waves; 19, 0 and 2 pair tiles (33 dirty cells)
    "w6_192": Spec(192, 67, (32, 32 * 66, 32 * 66 + 1), gap=40, seed=2),      # 6 waves; 1 pair tile (32 cells), n_tiles - 1, n_tiles (full list)
    "w4_120": Spec(120, 72, (700, 33), splits=(1, 3, 8, 9), seed=3),          # 4 waves, 9 windows
    "w4_128_k16": Spec(128, 64, (500, 0, 1000), k16=True, seed=4),            # 4 waves, fp16 K
    "w6_176_k16": Spec(176, 67, (500, 2100), k16=True, gap=8, seed=5),        # 6 waves, fp16 K, ragged last window
    "nw_384": Spec(384, 64, (300,), seed=6),                                  # attn32_nw = 4 | 6
    "trip_120": Spec(120, 64, (500, 800), trip=True, seed=7),                 # (batch, head 0) flagged for the re-run
}
