"""The three entry points VATLiDAR's cross-attention reaches k_attn32 through -- lvq_attention_bf16_tiled (TL = 1),
lvq_attention_bf16_tiled_signed (TL = 2 + k_attn_combine_signed + the predicated re-run) and lvq_attention_bf16_stream_totals (TL = 0 with
force_part + k_attn_combine_raw) -- through the C ABI against the fp64 references of tests/stream_route_cases.py: a peaked key stream
whose probes sit on the structural slots of the stream (tile, row-word window and KV-split edges), in clean cells, in computed rows and
in the table rows a signed batch has to subtract.  tests/test_stream_route_cases.py shows on the host that losing, not subtracting or
not adding any one probe moves its row by >= 8x the bound applied here.

Bounds are per element and come from fp64 quantities alone (stream_route_cases: "Bounds"); every check prints its largest err / bound.
Largest err / bound seen on an MI355X over all cases of this file: tiled 0.951 (plain query, one bf16 output: the output rounding alone
may reach 2^-8 |ref|, see below), signed 0.826, totals O / l 0.601, totals m + log2 l 0.003.  The unit roundoff of bf16 (8 significant
bits) is 2^-8, not 2^-9: 2^-9 is the error of a value at the top of its binade, a P just above a power of two is rounded by up to
2^-8 of itself.  So 2^-8 sum w |v| is the worst case of the P rounding itself rather than twice it, and R = 2^-9 |ref| is half of what
one bf16 output rounding can cost; the bounds are kept as they were set and hold with the figures above, but they have no factor of
two to spare.

Layouts are never the contiguous corner the wrappers in ops.py use: K and V are column blocks of a wider row (ldkv > 2 d; "wide": K and V
with a head stride of dh + 8 between padding columns), ldq > d, the output has o_hstride = dh + 8, ldo = H o_hstride + 24 and a gap
between batch elements; all operand padding holds PAD_VALUE (and `gap` unused rows between the table and the computed rows do), outputs,
totals and workspaces sit in canary-filled buffers that must keep their pattern outside the result / past the size passed.

Which k_attn32<NW, QS, TL, PIPE> a case launches follows from plan_k32_waves (176, 192 queries: 6 waves; 120, 128: 4; 384: 4 unless
attn32_nw = 6) and k32_pipe (4 waves: pipelined for QS != 0 or attn_pipe = 1, never with attn_pipe = -1; 6 waves: never) and is named in
each test's docstring.  The signed call always launches <NW, QS, 2, PIPE> and then <NW, QS, 1, PIPE> (the predicated re-run).
profiles/stream_routes_kernel_stats.csv is a kernel trace of this file: the 18 tiled / signed instantiations <4, q, t, false | true> and
<6, q, t, false> (q = 0, 1, 2; t = 1, 2), the totals' <4, 2, 0, false | true>, <6, 2, 0, false>, <4, 3, 0, false>, <6, 3, 0, false> (and
the QS = 0, 1 totals shared with lvq_attention_bf16), k_attn_combine, k_attn_combine_signed and k_attn_combine_raw."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import stream_route_cases as SC  # noqa: E402
from test_gpu_kernel_routes import DEV, EINVAL, EUNSUPPORTED, EWORKSPACE, OK, PAD_VALUE, Canary, F, addr, hi_lo, place  # noqa: E402

DH = SC.DH
BF = torch.bfloat16
assert PAD_VALUE == SC.PAD_VALUE


def _ptr(t, off=0):
    return 0 if t is None else t.data_ptr() + off * t.element_size()


# ------------------------------------------------------------------------------------------------
# device operands
# ------------------------------------------------------------------------------------------------
KV_LAYOUTS = {  # name -> (ldkv(d), K column, V column(d), head stride)
    "padded": (lambda d: 2 * d + 24, 0, lambda d: d, DH),                     # ldkv > 2 d, kv_hstride = dh
    "wide": (lambda d: 2 * d + 64, 16, lambda d: d + 40, DH + 8),             # K and V as column blocks of a wider row, padded heads
}


@functools.lru_cache(maxsize=4)
def kv_buffer(spec, layout):
    """ONE exactly sized K|V buffer in the given column layout; whatever is not K or V holds PAD_VALUE."""
    inp = SC.build(spec)
    d = spec.H * DH
    ld_f, kc, vc_f, hs = KV_LAYOUTS[layout]
    ld, vc = ld_f(d), vc_f(d)
    rows = inp.k.shape[0]
    buf = torch.full((rows, ld), PAD_VALUE, dtype=BF)
    kb = inp.k.half().view(BF) if spec.k16 else inp.k.to(BF)                  # fp16 K: IEEE fp16 bit patterns in the bf16 buffer
    vb = inp.v.to(BF)
    for h in range(spec.H):
        buf[:, kc + h * hs:kc + h * hs + DH] = kb[:, DH * h:DH * h + DH]
        buf[:, vc + h * hs:vc + h * hs + DH] = vb[:, DH * h:DH * h + DH]
    flat = buf.view(-1)[:(rows - 1) * ld + vc + (spec.H - 1) * hs + DH].contiguous().to(DEV)
    return SimpleNamespace(buf=flat, ld=ld, kc=kc, vc=vc, hs=hs)


@functools.lru_cache(maxsize=8)
def q_buffers(spec, batched):
    """(hi, lo, q_bstride, ldq): ldq = d + 16; one shared copy (q_bstride = 0) or one copy per batch element (q_bstride = nq * ldq)."""
    inp = SC.build(spec)
    d = spec.H * DH
    ldq = d + 16
    reps = spec.B if batched else 1
    hi, lo = hi_lo(inp.q.to(DEV))                                             # q is exactly hi + lo (stream_route_cases.build)
    mk = lambda t: place(t.unsqueeze(0).expand(reps, spec.nq, d), (spec.nq * ldq, ldq, 1))
    return mk(hi), mk(lo), (spec.nq * ldq if batched else 0), ldq


QFORM = {  # qform -> (pass q_lo, k_fp16 of the tiled / signed call, k_fp16 of the totals call)
    "plain": (False, 0, 0), "split": (True, 0, 0), "f16": (True, 1, 1), "f16x2": (True, None, 2),
}


def out_canaries(spec, want_lo, nq=None):
    nq = spec.nq if nq is None else nq
    o_hs = DH + 8
    ldo = spec.H * o_hs + 24
    o_bs = nq * ldo + 40
    mk = lambda: Canary(BF, (spec.B, nq, spec.H, DH), (o_bs, ldo, o_hs, 1), 64, 2 * ldo + 64)
    return mk(), (mk() if want_lo else None), (o_bs, ldo, o_hs)


def workspace(nbytes):
    return torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)


def ws_tail_ok(ws, nbytes):
    torch.cuda.synchronize()
    return bool((ws[nbytes:] == 0xA5).all())


def _v(x):
    return ctypes.c_void_p(x)


def _apply(e, ov):
    """Overrides of named arguments: a value, or a function of the value the call would have passed."""
    for name, val in ov.items():
        assert hasattr(e, name), name
        setattr(e, name, val(getattr(e, name)) if callable(val) else val)


# ------------------------------------------------------------------------------------------------
# the three calls; `ov` overrides named arguments (refusals), `ws_cut` passes that many bytes less than queried
# ------------------------------------------------------------------------------------------------
def call_totals(spec, qform, *, layout="padded", ws_cut=0, **ov):
    f = F()
    kv = kv_buffer(spec, layout)
    qh, ql, _, ldq = q_buffers(spec, False)
    use_lo, _, kf = QFORM[qform]
    tot = Canary(torch.float32, (spec.H, spec.nq, DH + 2), (spec.nq * (DH + 2), DH + 2, 1), 64, 64)
    e = SimpleNamespace(q=_ptr(qh), q_lo=_ptr(ql) if use_lo else 0, k=_ptr(kv.buf, kv.kc), v=_ptr(kv.buf, kv.vc), H=spec.H, nq=spec.nq, nkv=spec.nkv,
                        dh=DH, ldq=ldq, q_hs=DH, ldkv=kv.ld, kv_hs=kv.hs, k_fp16=kf, totals=tot.ptr().value)
    _apply(e, ov)
    nbytes = int(f.lib().lvq_attention_stream_totals_workspace_bytes(f.cint(spec.H), f.cint(spec.nq), f.cint(spec.nkv), f.cint(DH)))
    ws = workspace(nbytes)
    rc = f.lib().lvq_attention_bf16_stream_totals(_v(e.q), _v(e.q_lo), _v(e.k), _v(e.v), f.cint(e.H), f.cint(e.nq), f.cint(e.nkv), f.cint(e.dh), f.i64(e.ldq),
                                                  f.i64(e.q_hs), f.i64(e.ldkv), f.i64(e.kv_hs), f.cfloat(SC.SCALE), f.cint(e.k_fp16), _v(e.totals), addr(ws),
                                                  f.csize(nbytes - ws_cut), f.stream_ptr(torch.device(DEV)))
    assert ws_tail_ok(ws, nbytes - ws_cut), "the totals workspace was written past the size that was passed"
    return SimpleNamespace(rc=rc, tot=tot, ws_bytes=nbytes)


def _stream_env(spec, qform, layout, batched_q, want_lo, nq):
    kv = kv_buffer(spec, layout)
    qh, ql, q_bs, ldq = q_buffers(spec, batched_q)
    use_lo, kf, _ = QFORM[qform]
    o, ol, (o_bs, ldo, o_hs) = out_canaries(spec, want_lo, nq)
    src = SC.build(spec).row_src.to(DEV).contiguous()
    e = SimpleNamespace(q=_ptr(qh), q_lo=_ptr(ql) if use_lo else 0, k=_ptr(kv.buf, kv.kc), v=_ptr(kv.buf, kv.vc), row_src=_ptr(src), B=spec.B, H=spec.H,
                        nq=spec.nq if nq is None else nq, n_tiles=spec.n_tiles, dh=DH, q_bs=q_bs, ldq=ldq, q_hs=DH, ldkv=kv.ld, kv_hs=kv.hs, o_bs=o_bs,
                        ldo=ldo, o_hs=o_hs, k_fp16=kf, o=o.ptr().value, o_lo=ol.ptr().value if ol else 0)
    return e, o, ol, [src]


def call_tiled(spec, qform, *, layout="padded", batched_q=False, want_lo=None, ws_cut=0, nq=None, **ov):
    f = F()
    want_lo = (qform != "plain") if want_lo is None else want_lo
    e, o, ol, keep = _stream_env(spec, qform, layout, batched_q, want_lo, nq)
    _apply(e, ov)
    nbytes = int(f.lib().lvq_attention_workspace_bytes(f.cint(spec.B), f.cint(spec.H), f.cint(spec.nq), f.cint(spec.nkv), f.cint(DH), f.cint(1)))
    ws = workspace(nbytes)
    rc = f.lib().lvq_attention_bf16_tiled(_v(e.q), _v(e.q_lo), _v(e.k), _v(e.v), _v(e.row_src), f.cint(e.B), f.cint(e.H), f.cint(e.nq), f.cint(e.n_tiles),
                                          f.cint(e.dh), f.i64(e.q_bs), f.i64(e.ldq), f.i64(e.q_hs), f.i64(e.ldkv), f.i64(e.kv_hs), f.i64(e.o_bs), f.i64(e.ldo),
                                          f.i64(e.o_hs), f.cfloat(SC.SCALE), f.cint(e.k_fp16), _v(e.o), _v(e.o_lo), addr(ws), f.csize(nbytes - ws_cut),
                                          f.stream_ptr(torch.device(DEV)))
    assert ws_tail_ok(ws, nbytes - ws_cut), "the workspace was written past the size that was passed"
    return SimpleNamespace(rc=rc, o=o, ol=ol, ws_bytes=nbytes)


def call_signed(spec, qform, tot_t, *, layout="padded", batched_q=False, want_lo=None, ws_bytes=None, nq=None, cap_extra=0, with_stats=True, **ov):
    f = F()
    want_lo = (qform != "plain") if want_lo is None else want_lo
    e, o, ol, keep = _stream_env(spec, qform, layout, batched_q, want_lo, nq)
    cap = spec.n_tiles + cap_extra
    # what lies beyond a batch element's list is unspecified: it names a gap row (PAD_VALUE) where the buffer has one
    ps, pi = SC.build(spec).pair_lists(cap, fill_row=spec.nkv if spec.gap else 0)
    ps, pi = ps.to(DEV).contiguous(), pi.to(DEV).contiguous()
    stats = Canary(torch.int32, (4,), (1,), 64, 64)
    stats.result().zero_()
    e.__dict__.update(pair_src=_ptr(ps), pair_info=_ptr(pi), cap=cap, totals=_ptr(tot_t), stats=stats.ptr().value if with_stats else 0)
    _apply(e, ov)
    nbytes = int(f.lib().lvq_attention_tiled_signed_workspace_bytes(f.cint(spec.B), f.cint(spec.H), f.cint(spec.nq), f.cint(spec.n_tiles), f.cint(DH)))
    ws = workspace(nbytes)
    passed = nbytes if ws_bytes is None else ws_bytes
    rc = f.lib().lvq_attention_bf16_tiled_signed(_v(e.q), _v(e.q_lo), _v(e.k), _v(e.v), _v(e.row_src), _v(e.pair_src), _v(e.pair_info), f.cint(e.cap), _v(e.totals),
                                                 f.cint(e.B), f.cint(e.H), f.cint(e.nq), f.cint(e.n_tiles), f.cint(e.dh), f.i64(e.q_bs), f.i64(e.ldq), f.i64(e.q_hs),
                                                 f.i64(e.ldkv), f.i64(e.kv_hs), f.i64(e.o_bs), f.i64(e.ldo), f.i64(e.o_hs), f.cfloat(SC.SCALE), f.cint(e.k_fp16),
                                                 _v(e.o), _v(e.o_lo), _v(e.stats), addr(ws), f.csize(passed), f.stream_ptr(torch.device(DEV)))
    assert ws_tail_ok(ws, passed), "the signed workspace was written past the size that was passed"
    assert stats.untouched(), "a store outside the four statistics words"
    return SimpleNamespace(rc=rc, o=o, ol=ol, stats=stats.result().cpu().tolist(), ws_bytes=nbytes)


# ------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------
WORST = {}


def _note(kind, ratio):
    WORST[kind] = max(WORST.get(kind, 0.0), ratio)


def got_of(r):
    g = r.o.result().float().cpu().double()
    return g + r.ol.result().float().cpu().double() if r.ol is not None else g


def check_stream(label, spec, qform, r, signed_call=False, flagged=()):
    """Every batch element of a tiled / signed result against its fp64 reference, canaries included.  flagged: (batch, head) pairs the
    signed call redid over the full stream (judged by the tiled bound)."""
    assert r.rc == OK, (label, r.rc)
    assert r.o.untouched() and (r.ol is None or r.ol.untouched()), f"{label}: a store outside the attention result"
    got = got_of(r).view(spec.B, spec.nq, -1)
    assert bool(torch.isfinite(got).all()), label
    for b in range(spec.B):
        signed = signed_call and spec.signed(b)
        ref = SC.reference(spec, qform, b, signed)
        bound = ref.bound(r.ol is not None)
        for (fb, fh) in flagged:
            if fb == b:
                cols = slice(DH * fh, DH * fh + DH)
                bound[:, cols] = SC.reference(spec, qform, b, False).bound(r.ol is not None)[:, cols]
        err = (got[b] - ref.o).abs()
        ratio = float((err / bound).max())
        kind = "signed" if signed else "tiled"
        _note(kind, ratio)
        print(f"{label} b={b} ({kind}, {spec.scenes[b]} dirty): err {float(err.max()):.3e} bound {float(bound.max()):.3e} err/bound {ratio:.3f} "
              f"max|ref| {float(ref.o.abs().max()):.2f}")
        assert ratio <= 1.0, (label, b, ratio)


def check_totals(label, spec, qform, r):
    """(O | m | l): O / l within the tiled bound (fp32 output: no output rounding term), m + log2 l within nkv 2^-23."""
    assert r.rc == OK, (label, r.rc)
    assert r.tot.untouched(), f"{label}: a store outside the totals"
    t = r.tot.result().cpu().double()
    assert bool(torch.isfinite(t).all()), label
    ref = SC.totals_reference(spec, qform)
    o = (t[:, :, :DH] / t[:, :, DH + 1:]).transpose(0, 1).reshape(spec.nq, -1)
    ratio = float(((o - ref.o).abs() / ref.bound(False, r=0.0)).max())
    lse_err = float((t[:, :, DH] + torch.log2(t[:, :, DH + 1]) - ref.lse2).abs().max())
    lse_bound = spec.nkv * 2.0 ** -23
    _note("totals O/l", ratio)
    _note("totals lse", lse_err / lse_bound)
    print(f"{label}: totals O / l err/bound {ratio:.3f}; m + log2 l err {lse_err:.3e} bound {lse_bound:.3e}")
    assert ratio <= 1.0 and lse_err <= lse_bound, (label, ratio, lse_err)


def bits(c):
    return None if c is None else c.result().view(torch.int16 if c.es == 2 else torch.int32).clone()


def same_bits(x, y):
    return (x is None and y is None) or torch.equal(x, y)


def pipes_of(spec, tune_fields):
    """4 waves: the pipelined and the plain form (attn_pipe = 1, -1); 6 waves have one form."""
    six = spec.nq in (176, 192) or tune_fields.get("attn32_nw") == 6
    return (0,) if six else (1, -1)


def signed_flags(spec):
    """(batch, head) pairs a trip spec flags: head 0 of every signed batch element with dirty cells."""
    return [(b, 0) for b in range(spec.B) if spec.trip and spec.signed(b) and spec.scenes[b]]


# ------------------------------------------------------------------------------------------------
# tiled
# ------------------------------------------------------------------------------------------------
STREAM_CASES = [("w6_176", "plain"), ("w6_176", "split"), ("w6_192", "plain"), ("w6_192", "split"), ("w4_120", "plain"), ("w4_120", "split"),
                ("w4_128_k16", "f16"), ("w6_176_k16", "f16")]


@pytest.mark.parametrize("name,qform", STREAM_CASES)
def test_tiled_vs_fp64(name, qform, tune):
    """k_attn32<NW, QS, 1, PIPE> + k_attn_combine: NW = 6 for w6_*, 4 for w4_* (there PIPE = true and false, bit-equal); QS = 0 plain,
    1 split, 2 f16.  attn_nsplit 1 (direct store, no combine), 3, 8 and the plan's own (0: 8 splits, 9 at 72 tiles); 512 bytes less than
    the workspace queried under a forced split count must be refused (the query is exact then: one plan for both query kinds)."""
    spec = SC.SPECS[name]
    layout = "wide" if name in ("w6_192", "w4_128_k16") else "padded"
    for ns in (1, 3, 8, 0):
        outs = []
        for pipe in pipes_of(spec, {}):
            tune(attn_nsplit=ns, attn_pipe=pipe)
            r = call_tiled(spec, qform, layout=layout)
            check_stream(f"tiled {name} {qform} ns={ns} pipe={pipe}", spec, qform, r)
            outs.append((bits(r.o), bits(r.ol)))
        if len(outs) == 2:
            assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]), "pipelined != plain form"
        if ns > 1:
            short = call_tiled(spec, qform, layout=layout, ws_cut=512)
            assert short.rc == EWORKSPACE, (ns, short.rc)
            assert short.o.untouched(everything=True) and (short.ol is None or short.ol.untouched(everything=True)), "a refused call wrote to o"


@pytest.mark.parametrize("name,qform", [("w6_192", "split"), ("w4_120", "plain"), ("w4_128_k16", "f16")])
def test_tiled_shared_query_equals_per_batch_copies(name, qform, tune):
    """q_bstride = 0 against q_bstride = nq * ldq with identical copies, and one bf16 output against hi + lo outputs (hi is the same
    rounding of the same fp32 value): bit for bit.  <6, 1, 1>, <4, 0, 1>, <4, 2, 1, true>."""
    spec = SC.SPECS[name]
    tune(attn_nsplit=3)
    a = call_tiled(spec, qform, want_lo=True)
    b = call_tiled(spec, qform, want_lo=True, batched_q=True)
    c = call_tiled(spec, qform, want_lo=False, batched_q=True)
    for r in (a, b, c):
        check_stream(f"tiled {name} {qform}", spec, qform, r)
    assert same_bits(bits(a.o), bits(b.o)) and same_bits(bits(a.ol), bits(b.ol)) and same_bits(bits(a.o), bits(c.o))


# ------------------------------------------------------------------------------------------------
# totals
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,qform", [("w6_176", "plain"), ("w6_192", "split"), ("w4_120", "plain"), ("w4_120", "split"), ("w4_128_k16", "f16"),
                                        ("w4_128_k16", "f16x2"), ("w6_176_k16", "f16"), ("w6_176_k16", "f16x2")])
def test_totals_vs_fp64(name, qform, tune):
    """k_attn32<NW, QS, 0, PIPE> with force_part + k_attn_combine_raw, the (O | m | l) buffer looked at directly: QS = 0, 1, 2 and 3
    (f16x2: <4, 3, 0, false> and <6, 3, 0, false>, which have no pipelined form); 4 waves in both forms, bit-equal.  The workspace query
    is exact under a forced split count: 512 bytes less must be refused, totals untouched."""
    spec = SC.SPECS[name]
    layout = "wide" if name == "w6_192" else "padded"
    for ns in (1, 3, 8):
        outs = []
        for pipe in pipes_of(spec, {}):
            tune(attn_nsplit=ns, attn_pipe=pipe)
            r = call_totals(spec, qform, layout=layout)
            check_totals(f"totals {name} {qform} ns={ns} pipe={pipe}", spec, qform, r)
            outs.append(bits(r.tot))
        if len(outs) == 2:
            assert same_bits(*outs), "pipelined != plain form"
        short = call_totals(spec, qform, layout=layout, ws_cut=512)
        assert short.rc == EWORKSPACE and short.tot.untouched(everything=True)


# ------------------------------------------------------------------------------------------------
# signed
# ------------------------------------------------------------------------------------------------
def signed_run(spec, qform, **kw):
    layout = kw.pop("layout", "padded")
    t = call_totals(spec, qform, layout=layout)
    assert t.rc == OK and t.tot.untouched()
    return call_signed(spec, qform, t.tot.result(), layout=layout, **kw)


@pytest.mark.parametrize("name,qform", STREAM_CASES)
def test_signed_vs_fp64(name, qform, tune):
    """k_attn32<NW, QS, 2, PIPE> + k_attn_combine_signed (+ the predicated <NW, QS, 1, PIPE>, which finds nothing flagged), the totals from
    lvq_attention_bf16_stream_totals under the same tuning.  Pair lists: 19 | 0 | 2 tiles (w6_176: 600, 0, 33 dirty cells), 1 | n_tiles - 1
    | full list (w6_192: 32, 32 * 66 and 32 * 66 + 1 cells, row_base = 64 n_tiles + 40 with PAD_VALUE rows in between), 22 | 2 (w4_120),
    16 | 0 | 32 (w4_128_k16), 16 | 66 (w6_176_k16).  attn_nsplit 1, 3, 8 and 40 (more splits than any list but one has tiles: empty
    ranges); pair_cap_tiles = n_tiles and n_tiles + 5.  No row comes near a trigger: the statistics count nothing."""
    spec = SC.SPECS[name]
    layout = "wide" if name in ("w6_192", "w4_128_k16") else "padded"
    for ns in (1, 3, 8, 40):
        outs = []
        for pipe in pipes_of(spec, {}):
            tune(attn_nsplit=ns, attn_pipe=pipe)
            r = signed_run(spec, qform, layout=layout, cap_extra=5 if ns == 3 else 0)
            check_stream(f"signed {name} {qform} ns={ns} pipe={pipe}", spec, qform, r, signed_call=True)
            assert r.stats[0] == 0 and r.stats[1] == 0 and r.stats[3] == 0, r.stats
            outs.append((bits(r.o), bits(r.ol)))
        if len(outs) == 2:
            assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]), "pipelined != plain form"


@pytest.mark.parametrize("name,qform", [("w6_176", "split"), ("w4_120", "split")])
def test_signed_shared_query_and_optional_arguments(name, qform, tune):
    """q_bstride = 0 == per-batch copies; stats = NULL and a single bf16 output change no bit of o."""
    spec = SC.SPECS[name]
    tune(attn_nsplit=3)
    a = signed_run(spec, qform)
    b = signed_run(spec, qform, batched_q=True, with_stats=False)
    c = signed_run(spec, qform, want_lo=False)
    for r in (a, b, c):
        check_stream(f"signed {name} {qform}", spec, qform, r, signed_call=True)
    assert same_bits(bits(a.o), bits(b.o)) and same_bits(bits(a.ol), bits(b.ol)) and same_bits(bits(a.o), bits(c.o))
    assert b.stats == [0, 0, 0, 0]


@pytest.mark.parametrize("qform", ["plain", "split"])
def test_signed_flagged_pairs_equal_the_tiled_call(qform, tune):
    """trip_120: query 0 of head 0 has 16 nats on ONE table row that both batch elements replace -- what the subtraction leaves of its
    row sum is < 1/32 of the table's, so (b, 0) is flagged and redone over the full stream by the predicated <4, QS, 1, PIPE> launch: equal
    to the tiled call's bits under the same split count, in both 4-wave forms; head 1 stays signed and meets the signed bound;
    stats[1] counts the two pairs once each."""
    spec = SC.SPECS["trip_120"]
    flagged = signed_flags(spec)
    assert flagged == [(0, 0), (1, 0)]
    for ns in (1, 3):
        for pipe in (1, -1):
            tune(attn_nsplit=ns, attn_pipe=pipe)
            s = signed_run(spec, qform)
            check_stream(f"signed trip {qform} ns={ns} pipe={pipe}", spec, qform, s, signed_call=True, flagged=flagged)
            t = call_tiled(spec, qform)
            check_stream(f"tiled trip {qform} ns={ns} pipe={pipe}", spec, qform, t)
            assert s.stats[1] == len(flagged), s.stats
            for c_s, c_t in ((s.o, t.o), (s.ol, t.ol)):
                if c_s is None:
                    continue
                for b, h in flagged:
                    assert torch.equal(c_s.result()[b, :, h].view(torch.int16), c_t.result()[b, :, h].view(torch.int16)), (b, h)


# ------------------------------------------------------------------------------------------------
# forced wave counts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qform", ["plain", "split"])
@pytest.mark.parametrize("nw", [4, 6])
def test_forced_wave_count(nw, qform, tune):
    """attn32_nw on 384 queries (three 4-wave tiles or two 6-wave tiles): <nw, QS, TL, *> for TL = 0, 1, 2, each against fp64 (the two
    wave counts need not agree bit for bit); 4 waves in both forms."""
    spec = SC.SPECS["nw_384"]
    for pipe in pipes_of(spec, dict(attn32_nw=nw)):
        tune(attn32_nw=nw, attn_nsplit=3, attn_pipe=pipe)
        check_totals(f"totals nw={nw} {qform} pipe={pipe}", spec, qform, call_totals(spec, qform))
        check_stream(f"tiled nw={nw} {qform} pipe={pipe}", spec, qform, call_tiled(spec, qform))
        check_stream(f"signed nw={nw} {qform} pipe={pipe}", spec, qform, signed_run(spec, qform), signed_call=True)


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def _untouched(r):
    ok = r.o.untouched(everything=True) and (r.ol is None or r.ol.untouched(everything=True))
    return ok and (not hasattr(r, "stats") or r.stats == [0, 0, 0, 0])


def _untouched(r):
    ok = r.o.untouched(everything=True) and (r.ol is None or r.ol.untouched(everything=True))
    return ok and (not hasattr(r, "stats") or r.stats == [0, 0, 0, 0])


def test_refusals_write_nothing(tune):
    """The return codes of include/lvq.h for what the three entry points refuse -- misaligned pointers, dh != 64, fewer than 4096 keys,
    strides that are no multiple of 8 (inputs) or 4 (outputs), NULL operands, a short workspace -- with o, o_lo, stats and totals
    entirely untouched; nq == 0 returns LVQ_OK and writes nothing."""
    spec = SC.SPECS["w4_120"]
    tune(attn_nsplit=3)
    tot = call_totals(spec, "split")
    assert tot.rc == OK
    totals = tot.tot.result()
    d = spec.H * DH
    stream_refusals = [
        (dict(q=lambda p: p + 8), EUNSUPPORTED),                   # 8 bytes off a 16-byte boundary
        (dict(q_lo=lambda p: p + 8), EUNSUPPORTED),
        (dict(k=lambda p: p + 8), EUNSUPPORTED),
        (dict(v=lambda p: p + 8), EUNSUPPORTED),
        (dict(row_src=lambda p: p + 8), EUNSUPPORTED),
        (dict(o=lambda p: p + 4), EUNSUPPORTED),                   # 4 bytes off an 8-byte boundary
        (dict(o_lo=lambda p: p + 4), EUNSUPPORTED),
        (dict(dh=32), EUNSUPPORTED),
        (dict(dh=128), EUNSUPPORTED),
        (dict(n_tiles=63), EUNSUPPORTED),                          # 4032 keys: not a long-stream shape
        (dict(ldq=d + 4), EUNSUPPORTED),
        (dict(q_hs=DH + 4), EUNSUPPORTED),
        (dict(q_bs=12), EUNSUPPORTED),
        (dict(ldkv=lambda x: x + 4), EUNSUPPORTED),
        (dict(kv_hs=DH + 4), EUNSUPPORTED),
        (dict(ldo=lambda x: x + 2), EUNSUPPORTED),
        (dict(o_hs=DH + 2), EUNSUPPORTED),
        (dict(o_bs=lambda x: x + 2), EUNSUPPORTED),
        (dict(q=0), EINVAL),
        (dict(row_src=0), EINVAL),
        (dict(o=0), EINVAL),
        (dict(B=0), EINVAL),
    ]
    for ov, want in stream_refusals:
        for r in (call_tiled(spec, "split", **ov), call_signed(spec, "split", totals, **ov)):
            assert r.rc == want, (list(ov), r.rc, want)
            assert _untouched(r), ("a refused call wrote", list(ov))
    # signed only: NULL / misaligned totals and pair lists, no pair capacity, a workspace that cannot hold partials + flags
    for ov, want in ((dict(totals=0), EINVAL), (dict(totals=lambda p: p + 4), EUNSUPPORTED), (dict(pair_src=0), EINVAL),
                     (dict(pair_src=lambda p: p + 8), EUNSUPPORTED), (dict(pair_info=0), EINVAL), (dict(cap=0), EINVAL)):
        r = call_signed(spec, "split", totals, **ov)
        assert r.rc == want and _untouched(r), (list(ov), r.rc)
    # (the signed query also covers the statistics slots and alignment slack: it is not exact, so the cut is made at the partials)
    part = spec.B * spec.H * 3 * spec.nq * (DH + 2) * 4
    for nbytes in (part - 512, part):                              # the partials do not fit | the partials fit, the flags do not
        r = call_signed(spec, "split", totals, ws_bytes=nbytes)
        assert r.rc == EWORKSPACE and _untouched(r), nbytes
    for r in (call_tiled(spec, "split", nq=0), call_signed(spec, "split", totals, nq=0)):
        assert r.rc == OK and _untouched(r)
    # totals
    for ov, want in ((dict(totals=0), EINVAL), (dict(q=0), EINVAL), (dict(k=0), EINVAL), (dict(nq=0), EINVAL), (dict(dh=32), EUNSUPPORTED),
                     (dict(nkv=4032), EUNSUPPORTED), (dict(q=lambda p: p + 8), EUNSUPPORTED), (dict(k=lambda p: p + 8), EUNSUPPORTED),
                     (dict(ldq=d + 4), EUNSUPPORTED), (dict(ldkv=lambda x: x + 4), EUNSUPPORTED), (dict(kv_hs=DH + 4), EUNSUPPORTED),
                     (dict(q_hs=DH + 4), EUNSUPPORTED), (dict(totals=lambda p: p + 4), EUNSUPPORTED)):
        r = call_totals(spec, "split", **ov)
        assert r.rc == want, (list(ov), r.rc)
        assert r.tot.untouched(everything=True), ("a refused totals call wrote", list(ov))
