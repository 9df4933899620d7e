"""oracle/bev_tiles_oracle.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Host fp64 restatement of the sparse BEV key stream of VATLiDAR (include/lvq.h "sparse BEV key stream"; csrc/bev_tiles.hip), written
from the formulas of the header, not from the kernels:

  bookkeeping     pieces, dirty masks, compact row numbers (lvq_bev_tiles)
  conv_tokens     t = GELU_erf(b9 + depthwise 3 x 3 over the pillar canvas)                       (refine, vat_lidar.py:212-221)
  tile_tokens_ref x = LayerNorm(Wp t + bp) * gamma + beta + PE[key]                                (lvq_bev_tile_tokens)
  tile_kv_ref     K|V = rstd (M t + m0) + T[key],  rstd = 1 / sqrt((|R t + r0|^2 + c0) / d_ln + eps)   (lvq_bev_tile_kv)

Keys run tile-major: cell (y, x) is key 64 t + 8 p + 4 (y & 1) + (x & 3) with t the 8 x 8 tile and p = 2 ((y & 7) >> 1) + ((x & 7) >> 2)
its 2 x 4 piece; rows are in the compact (tile, scene, piece, cell) order of lvq_bev_tiles.

The references take the operands AS THE MODE SEES THEM: W / M / R are the values the kernel is given (bf16 values, or hi + lo summed), the
table T or PE exactly what it is given, and the conv token t is rounded here the way the mode rounds it:
  "plain"  t -> bf16(t)               "x3"  t -> hi + lo, hi = bf16(t), lo = bf16(t - hi)               "exact"  t as it is

Rounding ties.  The kernel forms t in fp32, the reference in fp64; where t lies at a bf16 rounding midpoint the two may round to
different neighbours and both are right.  near_midpoint() flags a (row, channel) whose fp64 value lies within 2^-20 * mag of a midpoint
between adjacent bf16 values, mag = |b9| + sum |v * w| being the size of the terms the conv adds up (fp32 unit roundoff 2^-24, about
ten chained operations, GELU's slope of at most 1.13).  judge_rows() evaluates every up / down variant of a row with one or two
flagged channels (at most 4) and accepts the row when it meets the tight bound against any of them; rows with three or more flagged
channels are held to the loose bound 2^-6 * max|ref| and counted.  With hi + lo operands the same flip moves hi + lo by 2^-17 relative,
far below the bounds, and nothing is flagged."""
from __future__ import annotations

import itertools
import math
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

TIE_WINDOW = 2.0 ** -20          # half width of the flagged band around a bf16 midpoint, relative to mag
LOOSE_REL = 2.0 ** -6            # bound of a row with three or more flagged channels, relative to max|ref|
LOOSE_SHARE = 0.005              # such rows must stay below this share of a case's rows


# ------------------------------------------------------------------------------------------------
# bookkeeping (lvq_bev_tiles)
# ------------------------------------------------------------------------------------------------
def dirty_cells(occ: np.ndarray) -> np.ndarray:
    """occ [B, H, W] bool -> [B, H, W] bool: a pillar in the 3 x 3 neighbourhood."""
    B, H, W = occ.shape
    pad = np.pad(occ, ((0, 0), (1, 1), (1, 1)))
    dirty = np.zeros((B, H, W), bool)
    for dy in range(3):
        for dx in range(3):
            dirty |= pad[:, dy:dy + H, dx:dx + W]
    return dirty


def bookkeeping(occ: np.ndarray, row_base: int, force_all: bool = False):
    """numpy restatement of lvq_bev_tiles: occ [B, H, W] bool -> (live codes, piece_dirty, row_src [B, HW], counts)."""
    B, H, W = occ.shape
    tw = W // 8
    nt = (H // 8) * tw
    dirty = np.ones((B, H, W), bool) if force_all else dirty_cells(occ)
    mask = np.zeros((B, nt, 8), np.int64)                                         # bit j = 4 cy + cx of piece p (rows 2 (p >> 1) .., columns 4 (p & 1) ..)
    for t in range(nt):
        for p in range(8):
            y0, x0 = (t // tw) * 8 + (p >> 1) * 2, (t % tw) * 8 + (p & 1) * 4
            for j in range(8):
                mask[:, t, p] |= dirty[:, y0 + (j >> 2), x0 + (j & 3)].astype(np.int64) << j
    codes, pdirty = [], []
    row_src = np.empty((B, nt * 64), np.int64)
    nd = 0
    for t in range(nt):
        for s in range(B):
            for p in range(8):
                m = int(mask[s, t, p])
                if m:
                    codes.append((t * B + s) * 8 + p)
                    pdirty.append((nd, m))
                for j in range(8):
                    e = 64 * t + 8 * p + j
                    if (m >> j) & 1:
                        row_src[s, e] = row_base + nd
                        nd += 1
                    else:
                        row_src[s, e] = e
    return codes, pdirty, row_src, (len(codes), 8 * len(codes), nd)


def rows_of(codes: Sequence[int], pdirty: Sequence[Tuple[int, int]], B: int, H: int, W: int) -> Dict[str, np.ndarray]:
    """The compact rows a (live list, piece_dirty) pair describes: per row its scene s, cell (y, x) and key, in row order.  Checks that
    the dirty-row numbers are consecutive in (piece, cell) order, as lvq_bev_tiles numbers them."""
    tw = W // 8
    s_, y_, x_, k_ = [], [], [], []
    for code, (first, m) in zip(codes, pdirty):
        assert first == len(s_), (first, len(s_))
        p, ts = code & 7, code >> 3
        t, s = ts // B, ts % B
        for j in range(8):
            if (m >> j) & 1:
                s_.append(s)
                y_.append((t // tw) * 8 + (p >> 1) * 2 + (j >> 2))
                x_.append((t % tw) * 8 + (p & 1) * 4 + (j & 3))
                k_.append(64 * t + 8 * p + j)
    a = lambda v: np.asarray(v, np.int64)
    return dict(s=a(s_), y=a(y_), x=a(x_), key=a(k_))


def key_of(y, x, W: int):
    """Tile-major key of cell (y, x): 64 t + 8 p + 4 (y & 1) + (x & 3)."""
    y, x = np.asarray(y), np.asarray(x)
    t = (y // 8) * (W // 8) + x // 8
    p = 2 * ((y & 7) >> 1) + ((x & 7) >> 2)
    return 64 * t + 8 * p + 4 * (y & 1) + (x & 3)


def tile_major(rows_hw: np.ndarray, H: int, W: int) -> np.ndarray:
    """[H*W, d] row-major cells -> the same rows in key order."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.empty_like(rows_hw)
    out[key_of(yy.ravel(), xx.ravel(), W)] = rows_hw
    return out


# ------------------------------------------------------------------------------------------------
# bf16 rounding of fp64 values (one rounding, nearest even -- not through fp32)
# ------------------------------------------------------------------------------------------------
def _ulp(x: np.ndarray, fmt: str = "bf16") -> np.ndarray:
    """Spacing of bf16 (8 significant bits) or IEEE fp16 (11) at |x|; values below the smallest normal share its spacing."""
    bits, emin = (8, -125) if fmt == "bf16" else (11, -13)
    _, e = np.frexp(x)
    return np.ldexp(1.0, np.maximum(e, emin) - bits)


def tight_bound(ref: np.ndarray, scale: float, a: float, fmt: str = "bf16") -> np.ndarray:
    """Elementwise bound of a correctly rounded result: the kernel rounds a value r' with |r' - ref| <= a * scale (everything before the
    final rounding: fp32 products and sums, `a` = 2e-5 plain / 2e-4 hi + lo operands) to the nearest bf16 / fp16 value, which moves it by
    at most half the spacing at r' -- so |got - ref| <= ulp(|ref| + a * scale) / 2 + a * scale.  Half a spacing is between 2^-9 |ref| (top
    of a binade) and 2^-8 |ref| (bottom) for bf16, 2^-12 .. 2^-11 for fp16; a result that is off by one whole spacing exceeds the bound
    wherever half a spacing exceeds a * scale.  The spacing is taken at |ref| + a * scale, so within a * scale below a power of two the
    bound uses the upper binade's spacing (r' may lie there): conservative by a factor of two on those few values."""
    return 0.5 * _ulp(np.abs(ref) + a * scale, fmt) + a * scale


def bf16_round(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, np.float64)
    u = _ulp(x)
    return np.rint(x / u) * u


def bf16_down_up(x: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    x = np.asarray(x, np.float64)
    u = _ulp(x)
    lo = np.floor(x / u) * u
    return lo, lo + u


def near_midpoint(t: np.ndarray, mag: np.ndarray) -> np.ndarray:
    """True where the fp64 value t lies within TIE_WINDOW * mag of a midpoint between adjacent bf16 values."""
    t = np.asarray(t, np.float64)
    u = _ulp(t)
    q = t / u
    return np.abs(q - np.floor(q) - 0.5) * u <= TIE_WINDOW * mag


def round_t(t: np.ndarray, mode: str) -> np.ndarray:
    if mode == "exact":
        return np.asarray(t, np.float64)
    hi = bf16_round(t)
    if mode == "plain":
        return hi
    assert mode == "x3", mode
    return hi + bf16_round(t - hi)


# ------------------------------------------------------------------------------------------------
# the formulas
# ------------------------------------------------------------------------------------------------
def gelu_erf(x: np.ndarray) -> np.ndarray:
    z = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return (0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))).numpy()


def conv_tokens(feat, coords, B: int, H: int, W: int, w9, b9):
    """feat [M, 64] pillar features, coords [M, 4] (scene, z, y, x), w9 [64, 9] (tap 3 dy + dx reads cell (y - 1 + dy, x - 1 + dx)),
    b9 [64] or None -> (t [B, H, W, 64] = GELU_erf(b9 + sum of the 9 taps), mag [B, H, W, 64] = |b9| + sum |v * w|), fp64; absent
    neighbours and the image border are zero."""
    feat, w9 = np.asarray(feat, np.float64), np.asarray(w9, np.float64)
    coords = np.asarray(coords)
    C = w9.shape[0]
    b = np.zeros(C) if b9 is None else np.asarray(b9, np.float64)
    canvas = np.zeros((B, H + 2, W + 2, C))
    canvas[coords[:, 0], coords[:, 2] + 1, coords[:, 3] + 1] = feat
    pre = np.broadcast_to(b, (B, H, W, C)).copy()
    mag = np.broadcast_to(np.abs(b), (B, H, W, C)).copy()
    for dy in range(3):
        for dx in range(3):
            term = canvas[:, dy:dy + H, dx:dx + W] * w9[:, 3 * dy + dx]
            pre += term
            mag += np.abs(term)
    return gelu_erf(pre), mag


def _take(t, rows):
    """t [B, H, W, C] and rows (dict of s, y, x, key) -> (t rows [n, C], keys); rows None: every cell, in (tile, scene, piece, cell) order."""
    t = np.asarray(t, np.float64)
    if rows is None:
        B, H, W, _ = t.shape
        codes, pdirty, _, _ = bookkeeping(np.zeros((B, H, W), bool), 0, force_all=True)
        rows = rows_of(codes, pdirty, B, H, W)
    return t[rows["s"], rows["y"], rows["x"]], rows["key"]


def tokens_rows(t_op, keys, Wp, bp, gamma, beta, eps, pe_tiled):
    """Row form of tile_tokens_ref: t_op [n, 64] as the kernel's product sees it."""
    f = lambda v: np.asarray(v, np.float64)
    y = t_op @ f(Wp).T + (0.0 if bp is None else f(bp))
    mu = y.mean(1, keepdims=True)
    var = ((y - mu) ** 2).mean(1, keepdims=True)
    return (y - mu) / np.sqrt(var + eps) * f(gamma) + (0.0 if beta is None else f(beta)) + f(pe_tiled)[keys]


def kv_rows(t_op, keys, M, m0, R, r0, c0, d_ln, eps, T):
    """Row form of tile_kv_ref: t_op [n, 64] as the kernel's products see it."""
    f = lambda v: np.asarray(v, np.float64)
    ss = ((t_op @ f(R).T + f(r0)) ** 2).sum(1, keepdims=True) + float(c0)
    rstd = 1.0 / np.sqrt(ss / float(d_ln) + eps)
    return rstd * (t_op @ f(M).T + f(m0)) + f(T)[keys]


def tile_tokens_ref(t, Wp, bp, gamma, beta, eps, pe_tiled, mode: str, rows=None):
    """LayerNorm(Wp t + bp) * gamma + beta + PE[key] of the rows `rows` (default: every cell) -> [n, N] fp64."""
    tr, keys = _take(t, rows)
    return tokens_rows(round_t(tr, mode), keys, Wp, bp, gamma, beta, eps, pe_tiled)


def tile_kv_ref(t, M, m0, R, r0, c0, d_ln, eps, T, mode: str, rows=None):
    """rstd (M t + m0) + T[key] of the rows `rows` (default: every cell) -> [n, 2 N] fp64."""
    tr, keys = _take(t, rows)
    return kv_rows(round_t(tr, mode), keys, M, m0, R, r0, c0, d_ln, eps, T)


# ------------------------------------------------------------------------------------------------
# judging kernel rows against the reference under the tie rule
# ------------------------------------------------------------------------------------------------
def flag_counts(t_rows, mag_rows, mode: str) -> np.ndarray:
    """Flagged channels per row (zero in every mode but "plain")."""
    if mode != "plain":
        return np.zeros(len(t_rows), np.int64)
    return near_midpoint(t_rows, mag_rows).sum(1)


def loose_share(t_rows, mag_rows, mode: str) -> float:
    n = flag_counts(t_rows, mag_rows, mode)
    return float((n >= 3).mean()) if len(n) else 0.0


def judge_rows(got: np.ndarray, t_rows: np.ndarray, mag_rows: np.ndarray, keys: np.ndarray, mode: str,
               ref_fn: Callable[[np.ndarray, np.ndarray], np.ndarray], tol_fn: Callable[[np.ndarray, float], np.ndarray]) -> Dict[str, float]:
    """got [n, D] kernel rows; ref_fn(t_op [m, 64], keys [m]) -> reference rows; tol_fn(ref, scale) -> elementwise tight bound with
    scale = max(1, max|ref|) of the case.  Returns the figures of the case:
      ratio  largest |got - ref| / bound over the rows held to the tight bound (best variant of a row with 1 or 2 flagged channels)
      err, bound   the largest error / bound pair of the rows without a flag;  loose_ratio  the largest error of the rows at the loose bound
      over that bound;  loose_rows, share  their number and share of the rows;  tie_rows  rows that were judged through variants."""
    got = np.asarray(got, np.float64)
    n = len(t_rows)
    out = dict(ratio=0.0, err=0.0, bound=0.0, loose_ratio=0.0, share=0.0, loose_rows=0, tie_rows=0, amax=0.0, rows=n)
    if n == 0:
        return out
    base = round_t(t_rows, mode)
    ref = ref_fn(base, keys)
    amax = float(np.abs(ref).max())
    scale = max(1.0, amax)
    out["amax"] = amax
    nf = flag_counts(t_rows, mag_rows, mode)
    err = np.abs(got - ref)
    ratio = err / tol_fn(ref, scale)
    row_ratio = ratio.max(1)
    tight = nf == 0
    ties = np.nonzero((nf >= 1) & (nf <= 2))[0]
    if len(ties):
        flg = near_midpoint(t_rows[ties], mag_rows[ties])
        dn, up = bf16_down_up(t_rows[ties])
        for r, row in enumerate(ties):
            ch = np.nonzero(flg[r])[0]
            best = row_ratio[row]
            for pick in itertools.product((0, 1), repeat=len(ch)):
                tv = base[row].copy()
                for c, u in zip(ch, pick):
                    tv[c] = up[r, c] if u else dn[r, c]
                rv = ref_fn(tv[None], keys[row:row + 1])[0]
                best = min(best, float((np.abs(got[row] - rv) / tol_fn(rv, scale)).max()))
            row_ratio[row] = best
        tight = tight | ((nf >= 1) & (nf <= 2))
        out["tie_rows"] = int(len(ties))
    if tight.any():
        w = np.nonzero(tight)[0]
        k = int(w[np.argmax(row_ratio[w])])
        out["ratio"] = float(row_ratio[k])
    if (nf == 0).any():                                          # the figures to print: the worst element of the rows without a flag
        w = np.nonzero(nf == 0)[0]
        k = int(w[np.argmax(ratio[w].max(1))])
        e = int(np.argmax(ratio[k]))
        out["err"], out["bound"] = float(err[k, e]), float(tol_fn(ref[k:k + 1], scale)[0, e])
    loose = nf >= 3
    if loose.any():
        out["loose_ratio"] = float(err[loose].max() / (LOOSE_REL * amax))
        out["share"], out["loose_rows"] = float(loose.mean()), int(loose.sum())
    return out
