"""GPU tests of the shared-prefix path (csrc/decode_shared.hip, lvq_qwen2_extend_shared, StandInHead.prefill_prefix /
generate(prefix=, prefix_index=), InferenceEngine.open_scene / Scene.ask / generate_batch(share_scenes=)), through the C ABI.

Bounds are those of the tests whose constructions are reused (tests/test_gpu_decode_ragged.py:4-6): 2e-5 with hi + lo operands and 8e-3 with
plain bf16 against fp32 softmax on the operands the kernel sees; 1e-4 / 2e-2 of max|ref| against oracle/decoder_oracle.py; logits within
1e-3 in bf16x3 and 2e-2 * max|scores| in bf16.  Where the issue asks for equal bits, bits are compared."""
import pytest
import torch

import cases
from conftest import golden

pytestmark = pytest.mark.gpu

from lidar_vision_vqa_amd import _ffi as F, synth  # noqa: E402
from oracle import decoder_oracle as DO  # noqa: E402
from test_gpu_decode_ragged import CUTS, _layer_struct, _prompts, _step_ragged  # noqa: E402
from test_gpu_head import build  # noqa: E402
from test_gpu_head_kernels import CANARY, GEO, bf16_pair, decoder_weights, gen  # noqa: E402,F401  (decoder_weights: module fixture)

DEV = "cuda:0"
NAN = float("nan")


def L():
    return F.lib()


def st():
    return F.stream_ptr(torch.device(DEV))


def i32(vals):
    return torch.tensor(list(vals), dtype=torch.int32, device=DEV)


def bits(t):
    return t.view(torch.int16)


def same(a, b):
    """bit-identical bf16 tensors, any NaN matching any NaN (padding rows are NaN on purpose)"""
    nan = torch.isnan(a) & torch.isnan(b)
    return bool(((bits(a) == bits(b)) | nan).all())


# ------------------------------------------------------------------------------------------------
# 1. the attention kernel
# ------------------------------------------------------------------------------------------------
def _cast3(t, split):
    """fp32 host [n, rows, w] -> device (hi, lo | None) of that shape, and what the kernel sees of it (fp32, host)"""
    from lidar_vision_vqa_amd import ops
    pair = tuple(None if p is None else p.view(t.shape) for p in ops.cast(t.reshape(-1, t.shape[-1]).contiguous().to(DEV), split))
    return pair, (pair[0].float() + (pair[1].float() if split else 0.0)).cpu()


def _mask_rows(pair, keep):
    """NaN in every row r >= keep[i] of pair[*][i]"""
    for part in pair:
        if part is not None:
            for i, n in enumerate(keep):
                part[i, n:] = NAN


def _case(dh, H, Hk, split, plens, pidx, own0, qn, lq, lown, seed):
    """Random q [B, lq], prefix caches [G, pmax] and own caches [B, lown] on the device, NaN behind every length, and the host values"""
    B, G, pmax = len(pidx), len(plens), max(plens)
    g = torch.Generator().manual_seed(seed)
    qd, q = _cast3(torch.randn(B, lq, H * dh, generator=g), split)
    pkd, pk = _cast3(torch.randn(G, pmax, Hk * dh, generator=g), split)
    pvd, pv = _cast3(torch.randn(G, pmax, Hk * dh, generator=g), split)
    kd, k = _cast3(torch.randn(B, lown, Hk * dh, generator=g), split)
    vd, v = _cast3(torch.randn(B, lown, Hk * dh, generator=g), split)
    _mask_rows(pkd, plens), _mask_rows(pvd, plens)
    _mask_rows(kd, [a + b for a, b in zip(own0, qn)]), _mask_rows(vd, [a + b for a, b in zip(own0, qn)])
    _mask_rows(qd, qn)
    return dict(dh=dh, H=H, Hk=Hk, split=split, plens=plens, pidx=pidx, own0=own0, qn=qn, lq=lq, lown=lown, dev=(qd, pkd, pvd, kd, vd),
                host=(q, pk, pv, k, v))


def _run(c, rows=None):
    """lvq_attention_extend_shared on the sub-batch `rows` of the case, in that order"""
    from lidar_vision_vqa_amd import ops
    qd, pkd, pvd, kd, vd = c["dev"]
    rows = list(range(len(c["pidx"]))) if rows is None else rows
    idx = torch.tensor(rows, device=DEV)
    sel = lambda pair: tuple(None if p is None else p.index_select(0, idx).contiguous() for p in pair)
    pick = lambda vals: i32(vals[r] for r in rows)
    return ops.attention_extend_shared(sel(qd), pkd, pvd, sel(kd), sel(vd), pick(c["pidx"]), i32(c["plens"]), pick(c["own0"]), pick(c["qn"]),
                                       n_heads=c["H"], n_kv_heads=c["Hk"], dh=c["dh"], scale=1.0 / c["dh"] ** 0.5)


PLENS = [1, 127, 128, 129, 840]
OWN = [0, 1, 62, 63, 64, 127, 128, 200]


@pytest.mark.parametrize("dh,H,Hk", [(64, 14, 2), (128, 6, 2), (64, 16, 1)])
@pytest.mark.parametrize("split", [False, True])
def test_one_query_row_equals_ragged_kernel_on_concatenated_caches(dh, H, Hk, split):
    """qn = 1: for prefix lengths 1, 127, 128, 129, 840 (two groups of different length per call) and 0 .. 200 cached own rows the output is
    BIT-IDENTICAL to lvq_attention_decode_ragged on caches that hold the prefix rows and the own rows one behind the other."""
    from lidar_vision_vqa_amd import ops
    lown = max(OWN) + 3
    for i, p0 in enumerate(PLENS):
        plens = [p0, PLENS[(i + 2) % len(PLENS)]]
        pidx = [j % 2 for j in range(len(OWN))]
        c = _case(dh, H, Hk, split, plens, pidx, OWN, [1] * len(OWN), 1, lown, 100 * i + dh + H)
        got = _run(c)
        qd, pkd, pvd, kd, vd = c["dev"]
        B, lmax = len(OWN), max(plens) + lown
        cat = lambda pre, own: tuple(None if p is None else torch.full((B, lmax, Hk * dh), NAN, dtype=torch.bfloat16, device=DEV) for p in pre)
        kc, vc = cat(pkd, kd), cat(pvd, vd)
        for b in range(B):
            n, m = plens[pidx[b]], OWN[b] + 1
            for dst, pre, own in ((kc, pkd, kd), (vc, pvd, vd)):
                for part in range(2 if split else 1):
                    dst[part][b, :n] = pre[part][pidx[b], :n]
                    dst[part][b, n:n + m] = own[part][b, :m]
        kv_len = i32(plens[pidx[b]] + OWN[b] + 1 for b in range(B))
        cs = (lmax * Hk * dh, Hk * dh, dh)
        flat = lambda pair: tuple(None if p is None else p.view(B, H * dh) for p in pair)
        ref = ops.attention_decode_ragged(flat(qd), kc, vc, kv_len, batch=B, n_heads=H, n_kv_heads=Hk, lmax=lmax, dh=dh,
                                          q_strides=(H * dh, H * dh, dh), k_strides=cs, v_strides=cs, scale=1.0 / dh ** 0.5)
        for part in range(2 if split else 1):
            assert bool(torch.isfinite(got[part].float()).all())
            assert torch.equal(bits(got[part].view(B, H * dh)), bits(ref[part])), (plens, part)


QN = [1, 2, 3, 17, 60, 9, 1]
QOWN = [0, 5, 0, 130, 0, 64, 199]
QIDX = [0, 1, 1, 0, 1, 0, 1]
QPLEN = [129, 840]


def _qcase(dh, H, Hk, split):
    return _case(dh, H, Hk, split, QPLEN, QIDX, QOWN, QN, max(QN), max(a + b for a, b in zip(QOWN, QN)) + 4, 7 * dh + H + Hk)


@pytest.mark.parametrize("dh,H,Hk", [(64, 4, 2), (128, 6, 2), (64, 14, 2), (64, 16, 1)])
@pytest.mark.parametrize("split", [False, True])
def test_ragged_query_chunks_vs_fp32_softmax(dh, H, Hk, split):
    """qn in {1, 2, 3, 17, 60} (and two sequences behind cached own rows) in one batch against softmax(q k^T / sqrt(dh)) v in fp32 on the
    operands the kernel sees, row by row over prefix rows + own rows up to the row itself: 2e-5 (hi + lo) / 8e-3 (bf16).  Every row of the
    prefix and own caches behind a length, and every padding query row, is NaN: finite results pin that none is read.  Rows r >= qn[b] come
    back as zeros, and no cache is written."""
    c = _qcase(dh, H, Hk, split)
    before = [None if p is None else p.clone() for pair in c["dev"][1:] for p in pair]
    out = _run(c)
    for a, b in zip(before, [p for pair in c["dev"][1:] for p in pair]):
        assert a is None or same(a, b)
    got = (out[0].float() + (out[1].float() if split else 0)).cpu()
    assert bool(torch.isfinite(got).all())
    q, pk, pv, k, v = c["host"]
    bound = 2e-5 if split else 8e-3
    worst = 0.0
    for b, (n, own, g) in enumerate(zip(QN, QOWN, QIDX)):
        for part in out[:2 if split else 1]:
            assert bool((bits(part[b, n:]) == 0).all()), ("padding rows are zero", b)
        heads = lambda t: t.view(-1, Hk, dh).permute(1, 0, 2).repeat_interleave(H // Hk, dim=0)
        for r in range(n):
            kk = heads(torch.cat([pk[g, :QPLEN[g]], k[b, :own + r + 1]]))
            vv = heads(torch.cat([pv[g, :QPLEN[g]], v[b, :own + r + 1]]))
            ref = (torch.softmax(q[b, r].view(H, 1, dh) @ kk.transpose(-1, -2) / dh ** 0.5, dim=-1) @ vv).reshape(H * dh)
            err = (got[b, r] - ref).abs().max().item()
            worst = max(worst, err)
            assert err < bound, (b, r, err)
    print(f"dh={dh} H={H} Hk={Hk} split={split}: max err {worst:.3g} (bound {bound:g})")


@pytest.mark.parametrize("dh,H,Hk", [(64, 14, 2), (128, 6, 2)])
@pytest.mark.parametrize("split", [False, True])
def test_extend_attention_is_batch_invariant(dh, H, Hk, split):
    """The output rows of a sequence in the batch of 7 equal, bit for bit, its rows alone (batch 1) and in a batch of 3 at another slot
    between sequences of other lengths and the other prefix: the work of a sequence depends on its own lengths only."""
    c = _qcase(dh, H, Hk, split)
    n = len(QN)
    full = _run(c)
    for b in range(n):
        alone = _run(c, [b])
        trio = _run(c, [(b + 4) % n, b, (b + 2) % n])
        for part in range(2 if split else 1):
            assert torch.equal(bits(full[part][b]), bits(alone[part][0])), (b, "alone", part)
            assert torch.equal(bits(full[part][b]), bits(trio[part][1])), (b, "batch of 3", part)


def test_extend_attention_bad_arguments():
    from lidar_vision_vqa_amd import ops
    c = _qcase(64, 4, 2, True)
    qd, pkd, pvd, kd, vd = c["dev"]
    args = lambda **kw: dict(dict(n_heads=4, n_kv_heads=2, dh=64, scale=0.125), **kw)
    v = [i32(c["pidx"]), i32(QPLEN), i32(QOWN), i32(QN)]
    with pytest.raises(F.LvqError):                             # hi + lo queries need hi + lo caches
        ops.attention_extend_shared(qd, (pkd[0], None), pvd, kd, vd, *v, **args())
    with pytest.raises(F.LvqError):                             # the lengths live on the device
        ops.attention_extend_shared(qd, pkd, pvd, kd, vd, v[0], v[1], v[2].cpu(), v[3], **args())
    with pytest.raises(F.LvqError):                             # a scale of 0
        ops.attention_extend_shared(qd, pkd, pvd, kd, vd, *v, **args(scale=0.0))


# ------------------------------------------------------------------------------------------------
# 2. the layer loop
# ------------------------------------------------------------------------------------------------
def _rows_cache(n, rows, filled, dkv, prec, g):
    """A cache [n, rows, dkv] (+ one guard row) of canaries with random entries in rows < filled[i]; device buffers (flat), their views and
    the fp64 values per sequence."""
    hi = torch.full(((n * rows + 1) * dkv,), CANARY, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    lo = hi.clone() if prec == 3 else None
    vals = []
    for i, m in enumerate(filled):
        h, l = bf16_pair(torch.randn(m, dkv, generator=g) * 1.5)
        hi[:n * rows * dkv].view(n, rows, dkv)[i, :m] = h.to(DEV)
        val = h.double()
        if prec == 3:
            lo[:n * rows * dkv].view(n, rows, dkv)[i, :m] = l.to(DEV)
            val = val + l.double()
        vals.append(val)
    return hi, lo, vals


def _prefix_struct(kh, kl, vh, vl):
    from lidar_vision_vqa_amd import head
    p = lambda t: None if t is None else t.data_ptr()
    return head._Qwen2PrefixPtrs(p(kh), p(kl), p(vh), p(vl))


def _extend(arr, parr, n_layers, xd, batch, lq, c, pidx, plen, pmax, own0, qn, t, lown, prec, ws=None):
    d, H, Hk, inter = c["d"], c["H"], c["Hk"], c["inter"]
    if ws is None:
        nbytes = int(L().lvq_qwen2_extend_shared_workspace_bytes(F.cint(batch), F.cint(lq), F.cint(d), F.cint(H), F.cint(Hk), F.cint(inter),
                                                                 F.cint(pmax), F.cint(lown), F.cint(prec)))
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    return L().lvq_qwen2_extend_shared(arr, parr, F.cint(n_layers), F.ptr(xd), F.cint(batch), F.cint(lq), F.cint(d), F.cint(H), F.cint(Hk),
                                       F.cint(inter), F.ptr(pidx), F.ptr(plen), F.cint(plen.numel()), F.cint(pmax), F.ptr(own0), F.ptr(qn),
                                       F.cint(t), F.cint(lown), F.cfloat(c["eps"]), F.cfloat(c["theta"]), F.cint(prec), F.ptr(ws),
                                       F.csize(ws.numel()), st())


def _shared_caches(decoder_weights, plens, own, lown, prec, g):
    """per layer: prefix caches [G, pmax] with plens rows and own caches [B, lown] with own[b] rows, + the structs"""
    from lidar_vision_vqa_amd import head
    c = GEO
    dkv = c["d"] // c["H"] * c["Hk"]
    G, B, pmax = len(plens), len(own), max(plens)
    arr, parr, caches = (head._Qwen2LayerPtrs * c["n_layers"])(), (head._Qwen2PrefixPtrs * c["n_layers"])(), []
    for i, (dw, _) in enumerate(decoder_weights):
        pk, pv = _rows_cache(G, pmax, plens, dkv, prec, g), _rows_cache(G, pmax, plens, dkv, prec, g)
        ok, ov = _rows_cache(B, lown, own, dkv, prec, g), _rows_cache(B, lown, own, dkv, prec, g)
        caches.append((pk, pv, ok, ov))
        arr[i] = _layer_struct(dw, prec, ok[0], ok[1], ov[0], ov[1])
        parr[i] = _prefix_struct(pk[0], pk[1], pv[0], pv[1])
    return arr, parr, caches


@pytest.mark.parametrize("prec", [1, 3])
def test_extend_shared_reference_geometry(decoder_weights, prec):
    """lvq_qwen2_extend_shared at the reference decoder's geometry (d 896, 14 / 2 heads, inter 4864; 2 layers): ragged query chunks of
    17, 5, 1 and 3 rows behind 0, 3, 130 and 0 cached own rows and two prefixes of 129 and 840 rows, against oracle/decoder_oracle.py run
    per sequence, row after row, on the concatenated history: 1e-4 (precision 3) / 2e-2 (precision 1) of max|ref| for the output rows and
    for the appended cache rows.  Canaries behind every length, the rows in front and the prefix caches stay as they were."""
    c = GEO
    d, H, Hk = c["d"], c["H"], c["Hk"]
    dkv = d // H * Hk
    plens, pidx, own, qn = [129, 840], [0, 1, 1, 0], [0, 3, 130, 0], [17, 5, 1, 3]
    B, lq, lown, pmax, t = len(qn), max(qn), 150, max(plens), 2
    rel = 1e-4 if prec == 3 else 2e-2
    g = gen(4711 + prec)
    arr, parr, caches = _shared_caches(decoder_weights, plens, own, lown, prec, g)
    before = [[None if buf is None else buf.clone() for pair in (layer[0], layer[1]) for buf in pair[:2]] for layer in caches]
    x = torch.randn(B, lq, d, generator=g)
    xd = x.clone()
    for b, n in enumerate(qn):
        xd[b, n:] = NAN                                                  # padding rows: whatever they hold stays out of the real rows
    xd = xd.to(DEV)
    # own0 + t is the number of cached own rows: the loop counter is part of the position
    rc = _extend(arr, parr, c["n_layers"], xd, B, lq, c, i32(pidx), i32(plens), pmax, i32(o - t for o in own), i32(qn), t, lown, prec)
    F.check(rc, "lvq_qwen2_extend_shared")
    got = xd.cpu().double()
    want_x, got_rows, want_rows = {}, {}, {}                             # the oracle: one sequence at a time, row after row
    for b in range(B):
        gi, P = pidx[b], plens[pidx[b]]
        hist = [(torch.cat([layer[0][2][gi], layer[2][2][b]]), torch.cat([layer[1][2][gi], layer[3][2][b]])) for layer in caches]
        for r in range(qn[b]):
            xb = x[b, r:r + 1].double()
            for i, (_, wr) in enumerate(decoder_weights):
                kh, vh = hist[i]
                xb, k_new, v_new = DO.decode_layer(xb, wr[prec], kh[None], vh[None], P + own[b] + r, H, Hk, c["eps"], c["theta"])
                hist[i] = (torch.cat([kh, k_new]), torch.cat([vh, v_new]))
                for which, new in ((2, k_new), (3, v_new)):
                    hi, lo, _ = caches[i][which]
                    row = hi[:B * lown * dkv].view(B, lown, dkv)[b, own[b] + r].cpu().double()
                    if prec == 3:
                        row = row + lo[:B * lown * dkv].view(B, lown, dkv)[b, own[b] + r].cpu().double()
                    got_rows.setdefault((i, which), []).append(row)
                    want_rows.setdefault((i, which), []).append(new[0])
            want_x[(b, r)] = xb[0]
    for key in want_rows:                                                # bounds relative to max|ref| of the whole tensor, as in the
        w, gr = torch.stack(want_rows[key]), torch.stack(got_rows[key])  # tests of the ragged step
        err = float((gr - w).abs().max())
        print(f"prec={prec} layer={key[0]} {'kv'[key[1] - 2]} rows: err {err:.3g} (bound {rel * float(w.abs().max()):.3g})")
        assert err <= rel * float(w.abs().max()), ("appended rows", key, err)
    w = torch.stack(list(want_x.values()))
    gx = torch.stack([got[b, r] for b, r in want_x])
    err = float((gx - w).abs().max())
    print(f"prec={prec}: output rows err {err:.3g} (bound {rel * float(w.abs().max()):.3g})")
    assert err <= rel * float(w.abs().max()), ("output rows", err)
    for i, layer in enumerate(caches):
        now = [buf for pair in (layer[0], layer[1]) for buf in pair[:2]]
        for a, bnow in zip(before[i], now):
            assert a is None or torch.equal(bits(a), bits(bnow)), ("prefix caches are read-only", i)
        for hi, lo, vals in (layer[2], layer[3]):
            for part in ((hi, lo) if prec == 3 else (hi,)):
                v = part[:B * lown * dkv].view(B, lown, dkv)
                for b in range(B):
                    assert bool((bits(v[b, own[b] + qn[b]:]) == CANARY).all()), ("rows behind the appended ones", i, b)
                assert bool((bits(part[B * lown * dkv:]) == CANARY).all()), ("guard row", i)
            for b in range(B):
                v = hi[:B * lown * dkv].view(B, lown, dkv)[b, :own[b]].cpu().double()
                if prec == 3:
                    v = v + lo[:B * lown * dkv].view(B, lown, dkv)[b, :own[b]].cpu().double()
                assert torch.equal(v, vals[b]), ("rows in front of the appended ones", i, b)


STEP_OWN = {1: [37], 3: [0, 63, 130], 8: [0, 1, 63, 127, 128, 129, 140, 5]}


@pytest.mark.parametrize("prec", [1, 3])
@pytest.mark.parametrize("batch", [1, 3, 8])
def test_one_row_step_equals_ragged_step_on_concatenated_caches(decoder_weights, batch, prec):
    """lq = 1, at most 8 sequences: the step takes the GEMV calls of lvq_qwen2_decode_step_ragged, and its output and the cache rows it
    appends are BIT-IDENTICAL to that step on caches that hold the prefix rows and the own rows one behind the other."""
    from lidar_vision_vqa_amd import head
    c = GEO
    d, H, Hk, inter = c["d"], c["H"], c["Hk"], c["inter"]
    dkv = d // H * Hk
    plens, own = [129, 840], STEP_OWN[batch]
    pidx = [b % 2 for b in range(batch)]
    lown, pmax, t = 150, max(plens), 3
    lmax = pmax + lown
    g = gen(99 * batch + prec)
    arr, parr, caches = _shared_caches(decoder_weights, plens, own, lown, prec, g)
    arr2, cats = (head._Qwen2LayerPtrs * c["n_layers"])(), []
    for i, (dw, _) in enumerate(decoder_weights):
        bufs = []
        for pre, ow in ((caches[i][0], caches[i][2]), (caches[i][1], caches[i][3])):
            for part in ((0, 1) if prec == 3 else (0,)):
                cat = torch.full((batch, lmax, dkv), CANARY, dtype=torch.int16, device=DEV).view(torch.bfloat16)
                pv, ovw = pre[part][:len(plens) * pmax * dkv].view(len(plens), pmax, dkv), ow[part][:batch * lown * dkv].view(batch, lown, dkv)
                for b in range(batch):
                    n = plens[pidx[b]]
                    cat[b, :n] = pv[pidx[b], :n]
                    cat[b, n:n + own[b]] = ovw[b, :own[b]]
                bufs.append(cat)
            if prec != 3:
                bufs.append(None)
        cats.append(bufs)
        arr2[i] = _layer_struct(dw, prec, *bufs)
    x = torch.randn(batch, d, generator=g)
    xa, xb = x.to(DEV), x.to(DEV)
    rc = _extend(arr, parr, c["n_layers"], xa, batch, 1, c, i32(pidx), i32(plens), pmax, i32(o - t for o in own), i32([1] * batch), t, lown, prec)
    F.check(rc, "lvq_qwen2_extend_shared")
    nbr = int(L().lvq_qwen2_decode_ragged_workspace_bytes(F.cint(batch), F.cint(d), F.cint(H), F.cint(Hk), F.cint(inter), F.cint(lmax), F.cint(prec)))
    pos0 = i32(plens[pidx[b]] + own[b] - t for b in range(batch))
    _step_ragged(arr2, c["n_layers"], xb, batch, dict(c, lmax=lmax), pos0, t, prec, torch.empty(nbr, dtype=torch.uint8, device=DEV))
    assert torch.equal(xa.view(torch.int32), xb.view(torch.int32))
    for i in range(c["n_layers"]):
        for j, ow in enumerate((caches[i][2], caches[i][3])):
            for part in ((0, 1) if prec == 3 else (0,)):
                ovw = ow[part][:batch * lown * dkv].view(batch, lown, dkv)
                for b in range(batch):
                    assert torch.equal(bits(ovw[b, own[b]]), bits(cats[i][2 * j + part][b, plens[pidx[b]] + own[b]])), (i, j, part, b)
                    assert bool((bits(ovw[b, own[b] + 1:]) == CANARY).all())


def test_extend_shared_rejects_and_clamps(decoder_weights):
    """What the host can see is LVQ_EINVAL; a sequence whose rows run past its own cache is clamped to the last row on the device: nothing
    is written outside its cache (guard row, the neighbour's rows)."""
    c = GEO
    dkv = c["d"] // c["H"] * c["Hk"]
    prec, plens, own, lown = 1, [40], [8, 2], 10
    g = gen(5)
    arr, parr, caches = _shared_caches(decoder_weights, plens, own, lown, prec, g)
    xd = torch.randn(2, 4, c["d"], generator=g).to(DEV)
    v = dict(pidx=i32([0, 0]), plen=i32(plens), own0=i32(own), qn=i32([4, 2]))
    call = lambda t=0, lq=4, **kw: _extend(arr, parr, c["n_layers"], xd, 2, lq, c, kw.get("pidx", v["pidx"]), v["plen"], 40,
                                           kw.get("own0", v["own0"]), v["qn"], t, lown, prec,
                                           ws=torch.empty(1 << 26, dtype=torch.uint8, device=DEV))
    assert call(t=-1) == -1 and call(t=lown) == -1 and call(lq=0) == -1
    F.check(call(), "lvq_qwen2_extend_shared")                       # sequence 0: rows 8, 9, then past the cache -> clamped to row 9
    for layer in caches:
        for hi, _, _ in (layer[2], layer[3]):
            vw = hi[:2 * lown * dkv].view(2, lown, dkv)
            assert bool((bits(hi[2 * lown * dkv:]) == CANARY).all())
            assert bool((bits(vw[1, 4:]) == CANARY).all()) and not bool((bits(vw[1, 3]) == CANARY).all())
            assert not bool((bits(vw[0, 9]) == CANARY).all())
    assert bool(torch.isfinite(xd[1, :2]).all())


# ------------------------------------------------------------------------------------------------
# 3. the head
# ------------------------------------------------------------------------------------------------
# The prompts of test_ragged_generate_equals_per_prompt_generate (CUTS: six cuts of the two golden prompts; smallest top-1 / top-2 logit
# margin over all sequences and the 12 greedy steps 0.1058 with the CPU oracle, i.e. 100x the bf16x3 logit bound of 1e-3), each split into
# a prefix -- the first PLEN[row] rows of its golden prompt -- and the rows behind it.
PLEN = {0: 25, 1: 28}


def _split_prompts():
    hc = cases.HEAD_CASE
    inp = torch.from_numpy(golden("head_prefix")["inputs_embeds"])[:, :-hc["n_answer"]].contiguous()
    pmax = max(PLEN.values())
    pre = torch.full((2, pmax, inp.shape[2]), NAN, device=DEV)                     # rows behind a prefix are garbage: prefill_prefix zeroes them
    for r, n in PLEN.items():
        pre[r, :n] = inp[r, :n]
    singles, batch, lens = _prompts()
    qlen = [int(n) - PLEN[r] for n, (r, _) in zip(lens.tolist(), CUTS)]
    rest = torch.full((len(CUTS), max(qlen), inp.shape[2]), NAN, device=DEV)
    for i, (s, (r, _)) in enumerate(zip(singles, CUTS)):
        rest[i, :qlen[i]] = s[0, PLEN[r]:]
    pidx = torch.tensor([r for r, _ in CUTS], device=DEV)
    return pre, torch.tensor([PLEN[0], PLEN[1]], device=DEV), rest, torch.tensor(qlen, device=DEV), pidx, batch, lens


@pytest.mark.parametrize("prec,tol", [("bf16x3", 1e-3), ("bf16", None)])
def test_generate_with_prefix_equals_generate_on_concatenated_prompts(prec, tol):
    """Six sequences behind two cached prefixes of different length against `generate(prompt_lengths=)` on the whole prompts: token ids equal
    for every sequence and step (smallest margin 0.1058, see above), per-step logits within the mode's bound, EOS / pad per sequence."""
    hc = cases.HEAD_CASE
    base = build(hc, prec)[0]
    n = golden("head_generate")["ids"].shape[1]
    pre, plen, rest, qlen, pidx, batch, lens = _split_prompts()
    ref_ids, ref_sc = base.generate(inputs_embeds=batch, prompt_lengths=lens, max_new_tokens=n, do_sample=False, pad_token_id=0,
                                    eos_token_id=None, output_scores=True)
    cache = base.prefill_prefix(pre, plen)
    assert cache.n_prefix == 2 and cache.lengths == [PLEN[0], PLEN[1]] and cache.pmax == max(PLEN.values())
    mask = (torch.arange(rest.shape[1], device=DEV)[None] < qlen[:, None]).long()
    bound = tol if tol is not None else 2e-2 * float(ref_sc.abs().max())
    for am in (None, mask):
        ids, sc = base.generate(inputs_embeds=rest, attention_mask=am, prompt_lengths=qlen, prefix=cache, prefix_index=pidx, max_new_tokens=n,
                                do_sample=False, pad_token_id=0, eos_token_id=None, output_scores=True)
        err = float((sc - ref_sc).abs().max())
        print(f"{prec}: with prefix vs whole prompts logits max err {err:.3g} (bound {bound:.3g})")
        assert ids.dtype == torch.int64 and tuple(ids.shape) == (len(CUTS), n)
        assert torch.equal(ids, ref_ids)
        assert err < bound, err
    assert bool(torch.isnan(rest).any()) and bool(torch.isnan(pre).any())            # the inputs are not modified
    for eos in (500, 467):
        hit = [(r.index(eos) if eos in r else None) for r in ref_ids.tolist()]
        assert any(h is not None for h in hit) and any(h is None for h in hit)
        ids2 = base.generate(inputs_embeds=rest, prompt_lengths=qlen, prefix=cache, prefix_index=pidx, max_new_tokens=n, do_sample=False,
                             pad_token_id=0, eos_token_id=eos)
        want = ref_ids.clone()
        for b, h in enumerate(hit):
            if h is not None:
                want[b, h + 1:] = 0
        assert torch.equal(ids2, want), eos
    # one prefix, no prefix_index, no prompt_lengths: the sequences of group 0 that are uncut
    one = base.prefill_prefix(pre[:1, :PLEN[0]].contiguous())
    ids3 = base.generate(inputs_embeds=rest[:1, :int(qlen[0])].contiguous(), prefix=one, max_new_tokens=n, do_sample=False)
    assert torch.equal(ids3, ref_ids[:1])


def test_prefix_cache_is_bound_to_head_weights_and_mode(monkeypatch):
    hc = cases.HEAD_CASE
    base = build(hc, "bf16x3")[0]
    other = build(hc, "bf16x3")[0]
    pre, plen, rest, qlen, pidx, _, _ = _split_prompts()
    cache = base.prefill_prefix(pre, plen)
    kw = dict(inputs_embeds=rest, prompt_lengths=qlen, prefix=cache, prefix_index=pidx, max_new_tokens=2, do_sample=False)
    assert tuple(base.generate(**kw).shape) == (len(CUTS), 2)
    with pytest.raises(F.LvqError):                              # another head, although its weights are equal
        other.generate(**kw)
    with pytest.raises(F.LvqError):                              # beam search stays unbuilt
        base.generate(**dict(kw, num_beams=2))
    with pytest.raises(F.LvqError):                              # several prefixes need prefix_index
        base.generate(**dict(kw, prefix_index=None))
    with pytest.raises(F.LvqError):
        base.generate(**dict(kw, prefix_index=pidx + 1))
    with pytest.raises(F.LvqError):
        base.generate(**dict(kw, prefix=None))                   # prefix_index without a prefix
    monkeypatch.setenv("LVQ_DECODE_PYTHON", "1")
    with pytest.raises(F.LvqError):
        base.generate(**kw)
    monkeypatch.delenv("LVQ_DECODE_PYTHON")
    base.precision = "bf16"
    with pytest.raises(F.LvqError):                              # another precision mode
        base.generate(**kw)
    base.precision = "bf16x3"
    assert tuple(base.generate(**kw).shape) == (len(CUTS), 2)
    with torch.no_grad():
        base.model.layers[1].mlp.down_proj.weight.mul_(1.0)      # a weight update (the values do not matter: the version does)
    with pytest.raises(F.LvqError):
        base.generate(**kw)
    assert tuple(base.generate(**dict(kw, prefix=base.prefill_prefix(pre, plen))).shape) == (len(CUTS), 2)


# ------------------------------------------------------------------------------------------------
# 4. the engine
# ------------------------------------------------------------------------------------------------
# (question, BEV seed offset = scene): three scenes with 1, 3 and 4 questions, interleaved.  With the CPU oracles (oracle/vat_oracle.py:
# vat_lidar + qwen2_generate, fp32) the smallest top-1 / top-2 margin over the 6 greedy steps of these eight prompts is 0.1193 (in input
# order: 0.1417, 0.1391, 0.1686, 0.1383, 0.1288, 0.1193, 0.9552, 0.5270), i.e. more than 100x the bf16x3 logit bound of 1e-3.  Questions
# with thinner margins on their BEV (e.g. "Is the road wet?" on scene 42: 0.0556) were left out.
SCENE_Q = [("Count the cyclists.", 40), ("Is it safe to turn left at the next junction?", 42), ("Is it safe to turn left at the next junction?", 41),
           ("Any obstacles?", 40), ("Any trucks?", 42), ("Any obstacles?", 42), ("How many cars are ahead of the ego vehicle?", 40),
           ("How many lanes are there?", 42)]


class Counting:
    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, x, *a, **kw):
        self.calls.append(tuple(x.shape))
        return self.fn(x, *a, **kw)


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_engine_share_scenes_equals_the_per_question_loop(prec, monkeypatch):
    """generate_batch(share_scenes=True) returns the strings of generate_batch(batch_size=1) in greedy mode for three scenes with 1, 3 and 4
    questions interleaved in the input (margins: see SCENE_Q), in one group, in groups of 3 and through open_scene / Scene.ask; the LiDAR
    encoder runs once per scene and prefill_prefix sees sum(P) rows."""
    from lidar_vision_vqa_amd import engine
    hc = cases.HEAD_CASE
    base, vl, va, vv = build(hc, prec)
    tok = synth.DummyTokenizer(hc["vocab"])
    lidar = Counting(vl)
    eng = engine.InferenceEngine(dict(tokenizer=tok, base_model=base, vat_lidar=lidar, device=torch.device(DEV), d_model=hc["d"],
                                      config=dict(use_vision=False, prefix_scale=0.2)))
    bevs = {s: synth.randn((16, 10, 10), hc["seed"] + s) for s in (40, 41, 42)}
    qs = [q for q, _ in SCENE_Q]
    bs = [bevs[s] for _, s in SCENE_Q]
    ts = [f"sample-{s}" for _, s in SCENE_Q]
    loop = eng.generate_batch(qs, bs, ts, max_new_tokens=6, do_sample=False)
    assert len(loop) == 8 and all(len(a) == 6 for a in loop) and len(set(loop)) >= 4
    assert len(lidar.calls) == 8
    prefill = Counting(base.prefill_prefix)
    monkeypatch.setattr(base, "prefill_prefix", prefill, raising=False)
    P = 2 + hc["nq_lidar"]
    for batch_size, tokens in ((8, ts), (3, ts), (16, None)):
        lidar.calls.clear(), prefill.calls.clear()
        got = eng.generate_batch(qs, bs, tokens, batch_size, share_scenes=True, max_new_tokens=6, do_sample=False)
        assert got == loop, (batch_size, got, loop)
        assert lidar.calls == [(1, 16, 10, 10)] * 3                                # one LiDAR pass per scene
        assert sum(c[0] * c[1] for c in prefill.calls) == 3 * P and len(prefill.calls) == 3
    lidar.calls.clear()
    scene = eng.open_scene(bevs[42], "sample-42")
    assert scene.n_rows == P
    mine = [i for i, (_, s) in enumerate(SCENE_Q) if s == 42]
    assert scene.ask([qs[i] for i in mine], max_new_tokens=6, do_sample=False) == [loop[i] for i in mine]
    assert scene.ask([qs[mine[1]]], max_new_tokens=6, do_sample=False) == [loop[mine[1]]]
    assert len(lidar.calls) == 1
    a = scene.ask(qs[:3], max_new_tokens=6, generator=torch.Generator(device=DEV).manual_seed(7))
    b = scene.ask(qs[:3], max_new_tokens=6, generator=torch.Generator(device=DEV).manual_seed(7))
    assert a == b and len(a) == 3
    with pytest.raises(F.LvqError):
        eng.generate_batch(qs, bs, ts, 8, share_scenes=True, max_new_tokens=6, do_sample=False, num_beams=4)
