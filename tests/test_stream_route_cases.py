"""The conditions under which the inputs of tests/stream_route_cases.py can tell a wrong long-stream kernel from a right one -- "this
test would notice", asserted on the host in fp64 (no GPU): every probe holds real softmax mass, losing any one probe key (or not
subtracting / not adding one in the signed stream) moves its row by many times the bound the GPU test applies, every structural slot of
the stream is somebody's probe, and a kernel that rounds P to bf16 stays inside the bound."""
import pytest
import torch

import stream_route_cases as SC

CASES = [(name, "f16" if spec.k16 else qf) for name, spec in SC.SPECS.items() for qf in (("plain", "split") if not spec.k16 else ("f16",))]


def _rows(spec):
    """[H, nq] mask of the rows that carry the three 10-nat probes (all but the trip row)."""
    ok = torch.ones(spec.H, spec.nq, dtype=torch.bool)
    if spec.trip:
        ok[0, 0] = False
    return ok


def _row_bound(ref, spec, out_lo):
    """Largest bound over the 64 outputs of each (head, query) row -> [H, nq]"""
    return ref.bound(out_lo).view(spec.nq, spec.H, SC.DH).amax(-1).t()


@pytest.mark.parametrize("name,qform", CASES)
def test_probes_carry_mass_and_losing_one_is_seen(name, qform):
    spec = SC.SPECS[name]
    ok = _rows(spec)
    for b in range(spec.B):
        for signed in ((False, True) if (spec.signed(b) and spec.scenes[b]) else (False,)):
            ref = SC.reference(spec, qform, b, signed)
            bound = _row_bound(ref, spec, out_lo=False)                          # the larger of the two output bounds
            flagged_head0 = spec.trip and signed
            for probe, mass, moved in SC.probe_effects(spec, qform, b, signed):
                sel = ok.clone()
                if flagged_head0:
                    sel[0] = False                                               # redone over the full stream: judged as tiled rows
                if mass is not None:
                    assert float(mass[sel].min()) >= 0.05, (name, b, probe, float(mass[sel].min()))
                worst = float((moved / bound)[sel].min())
                assert worst >= 8.0, (name, b, signed, probe, worst)


@pytest.mark.parametrize("name", list(SC.SPECS))
def test_structural_slots_are_probed(name):
    spec = SC.SPECS[name]
    inp = SC.build(spec)
    ok = _rows(spec)
    probed = set(inp.probe_a[ok].tolist())
    nt, nkv = spec.n_tiles, spec.nkv
    want = {0, nkv - 1, 63, 64}
    want |= {x for t in range(8, nt, 8) for x in (64 * t - 1, 64 * t)}
    for ns in spec.splits:
        tps = -(-nt // ns)
        want |= {x for sp in range(1, ns) if sp * tps < nt for x in (64 * sp * tps - 1, 64 * sp * tps)}
    if nt % 8:
        want.add(64 * (nt - 1))
    assert want <= probed, sorted(want - probed)
    # structural slots are clean everywhere; C and S cells are dirty in every scene that has dirty cells; nothing gathers a gap row
    for b, n in enumerate(spec.scenes):
        src = inp.row_src[b]
        assert int((src >= spec.row_base).sum()) == n
        assert bool((src[inp.slots] == torch.tensor(inp.slots, dtype=torch.int32)).all())
        assert not bool(((src >= nkv) & (src < spec.row_base)).any())
        if n:
            assert bool((src[inp.c_cells] >= spec.row_base).all()) and bool((src[inp.s_cells] >= spec.row_base).all())
    assert len(set(inp.probe_a[0].tolist()) | set(inp.c_cells.tolist()) | set(inp.s_cells.tolist())) == len(set(inp.probe_a[0].tolist())) + SC.N_C + SC.N_S


@pytest.mark.parametrize("name,qform", CASES)
def test_signed_rows_keep_clear_of_the_triggers(name, qform):
    """l_final / l_table of every judged row: two of the three probes stay (A, and C for S), so it sits near 1 -- at least 2x above the 1/16
    re-run trigger and below the 1.5x statistics trigger (which changes no result).  The trip row is at least 2x BELOW 1/16."""
    spec = SC.SPECS[name]
    ok = _rows(spec)
    for b in range(spec.B):
        if not (spec.signed(b) and spec.scenes[b]):
            continue
        r = SC.reference(spec, qform, b, True).ratio
        assert float(r[ok].min()) >= 2.0 / 16 and float(r[ok].max()) <= 1.25, (name, b, float(r[ok].min()), float(r[ok].max()))
        if spec.trip:
            assert float(r[0, 0]) <= 1.0 / 32, float(r[0, 0])


@pytest.mark.parametrize("name,qform", CASES)
def test_bf16_p_emulation_meets_the_bound(name, qform):
    spec = SC.SPECS[name]
    worst = 0.0
    for b in range(spec.B):
        for signed in ((False, True) if (spec.signed(b) and spec.scenes[b]) else (False,)):
            ref = SC.reference(spec, qform, b, signed)
            for out_lo in (False, True):
                got = SC.emulate_bf16_p(spec, qform, b, signed, out_lo)
                ratio = float(((got - ref.o).abs() / ref.bound(out_lo)).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (name, b, signed, out_lo, ratio)
    print(f"{name} {qform}: bf16-P emulation reaches {worst:.2f} of the bound")


def test_scores_reach_the_rescale_range():
    """The probes score 10 nats = 14.4 in log2 units, far above the deferred-rescale threshold of 6 that N(0, 1) inputs never reach, and
    the outputs are O(1) instead of 0.14."""
    spec = SC.SPECS["w6_176"]
    ref = SC.reference(spec, "plain", 0)
    assert float(SC._scores(spec, "plain").max()) > 14.0 and float(ref.o.abs().max()) > 1.0


def test_pair_lists_follow_the_documented_layout():
    spec = SC.SPECS["w6_192"]
    inp = SC.build(spec)
    ps, pi = inp.pair_lists(spec.n_tiles + 3, fill_row=spec.nkv)
    assert pi.tolist() == [[1, 1], [spec.n_tiles - 1, 1], [0, 0]]
    for b in (0, 1):
        n = spec.scenes[b]
        rows, cells = ps[b, :, :32].reshape(-1)[:n], ps[b, :, 32:].reshape(-1)[:n].long()
        assert bool((cells[1:] > cells[:-1]).all()) and bool((inp.row_src[b, cells] == rows).all()) and bool((rows >= spec.row_base).all())
        assert bool((ps[b, int(pi[b, 0]):] == spec.nkv).all())
