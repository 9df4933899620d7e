"""Every scene of the batch bench.py measures, in every mode it times, at BASELINE configs[1]'s full size (32 scenes of 32 768 points,
512 x 512 BEV = 262 144 keys, d = 768, 12 heads).  The other full-size tests run one scene; a 32-scene batch is where offsets pass 32 bits
(each layer's K|V buffer is [HW + 32 HW, 2d] bf16 = 26.6 GB: the computed rows' element offsets pass 2^31 from about scene 16 on
Dist-C and 2^32 before the batch ends on Dist-U) and where kernel choices follow the batch (KV split counts, XCD grouping, GEMM tile
families, scenes grouped by four).

  A  position equivariance: the batch reversed gives the same outputs, permuted, bit for bit (same B -> the same kernel choices; only
     the scenes' positions move): four modes on Dist-C, `mixed` on Dist-U and at n_layers = 4
  B  a scene run alone equals the same scene inside the batch, bit for bit, with the batch-dependent kernel choices pinned; the batch
     sizes run on one module as B = 1 -> 13 -> 32 -> 1, so the K|V buffers grow twice and the large ones are reused
  C  scene 31 at position 31 against the CPU oracle at the north-star 1e-3 (Dist-C and Dist-U)
  D  the dense-canvas input (VATLiDAR.forward(bev)) at the bench's B = 8 equals the sparse pillar input bit for bit

Inputs come from pipeline.synthetic_batch with the bench's seeds (Dist-C and L = 4: 1100 + i, Dist-U: 1002 + i); scene i alone is the
i-th per-scene array of that batch (synthetic_batch seeds every scene on its own, so it is synthetic_batch(cfg, 1, seed0 + i))."""

import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S = 32
TOL = 1e-3
MODES = ("mixed", "mixed16", "bf16", "bf16x3")
# B: the kernel choices that follow M or B, held fixed.  attn_nsplit: the KV split count of every attention kernel (plan_attn in
# csrc/attention.hip picks it from batch x heads x query tiles); 4 is at most the fuse block's 4 key tiles (196 keys), above which the
# override would be ignored there.  gemm_no256: the 256-row GEMM tile families, picked by M.  Everything else is chosen per scene or by
# shapes a batch does not change: the long-stream wave count and pipelined form (nq, nkv, query kind), each scene's signed / unsigned
# stream and its tile range per split (its own pair list, capacity n_tiles per scene), the 64 / 128-row GEMM tiles (same MFMA and k order
# per output element), the GEMV (M <= 8: no GEMM here is that short) and k_gemm_ln_rows (per scene the same row arithmetic).  No work
# split follows a quantity shared by the whole batch, so every comparison of B is bit-exact: none needs the accumulation-order bound.
PINNED = dict(attn_nsplit=4, gemm_no256=1)
SEED_C, SEED_U = 1100, 1002


def _cfg(**kw):
    from lidar_vision_vqa_amd import pipeline as P
    return P.PipelineConfig(**kw)


def _batch(pts_np, patches_np, order):
    """Device inputs of the scenes `order` (indices into the per-scene arrays of synthetic_batch), in that order."""
    pts = [pts_np[i] for i in order]
    off = np.concatenate(([0], np.cumsum([len(p) for p in pts]))).astype(np.int32)
    return (torch.from_numpy(np.concatenate(pts)).to(DEV), torch.from_numpy(off).to(DEV),
            torch.from_numpy(np.ascontiguousarray(patches_np[list(order)])).to(DEV))


def _scene(out, pos):
    """Per-scene outputs of the scene at batch position `pos`; the batch column of the coordinates is split off."""
    po = out["scene_pillar_off"].tolist()
    vo = out["scene_voxel_off"].tolist()
    pc = out["pillar_coords"][po[pos]:po[pos + 1]]
    vc = out["voxel_coords"][vo[pos]:vo[pos + 1]]
    return {"fused": out["fused"][pos], "lidar_tokens": out["lidar_tokens"][pos],
            "pillar_coords": pc[:, 1:], "pillar_batch": pc[:, 0], "pillar_features": out["pillar_features"][po[pos]:po[pos + 1]],
            "voxel_coords": vc[:, 1:], "voxel_batch": vc[:, 0], "voxel_num_points": out["voxel_num_points"][vo[pos]:vo[pos + 1]],
            "voxel_features": out["voxel_features"][vo[pos]:vo[pos + 1]]}


def _diff(a, pos_a, b, pos_b):
    """Names of the per-scene outputs that differ (bit for bit) between position pos_a of `a` and pos_b of `b`, plus a wrong batch column."""
    sa, sb = _scene(a, pos_a), _scene(b, pos_b)
    bad = [k for k in sa if not k.endswith("_batch") and not torch.equal(sa[k], sb[k])]
    for s, p, tag in ((sa, pos_a, "a"), (sb, pos_b, "b")):
        for k in ("pillar_batch", "voxel_batch"):
            if s[k].numel() == 0 or not bool((s[k] == p).all()):
                bad.append(f"{k}[{tag}] != {p}")
    return bad


def _tripped(pipe):
    return getattr(pipe.vat_lidar, "_guard_tripped", None)


def _kv_keys(pipe):
    return [k for k in pipe.vat_lidar._pe_cache if isinstance(k, tuple) and k[0] == "kv_buffer"]


def _kv_rows(pipe):
    """Row capacity of VATLiDAR's cached K|V buffers (the per-model table + the computed rows of the largest batch seen)."""
    keys = _kv_keys(pipe)
    assert len(keys) == 1
    return pipe.vat_lidar._pe_cache[keys[0]][1][0].shape[0]


@pytest.fixture(scope="module")
def state():
    """The full-size pipelines and batches, built once for the module; everything is freed at teardown (the K|V caches hold tens of GB)."""
    st = {}
    yield st
    st.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _get(st, name):
    from lidar_vision_vqa_amd import pipeline as P
    if name not in st:
        if name == "pipe":                      # bench.py's pipeline: FusionPipeline(PipelineConfig()), also timed on the Dist-U batch
            st[name] = P.FusionPipeline(_cfg(), DEV, precision="mixed")
        elif name == "pipe4":                   # value_n_layers_4
            st[name] = P.FusionPipeline(_cfg(n_layers=4), DEV, precision="mixed")
        elif name == "C":
            st[name] = P.synthetic_batch(_cfg(), S, SEED_C, DEV)
        elif name == "U":
            st[name] = P.synthetic_batch(_cfg(dist="U"), S, SEED_U, DEV)
        elif name == "L4":
            st[name] = P.synthetic_batch(_cfg(n_layers=4), 8, SEED_C, DEV)
    return st[name]


def _mixed_out(st, dist):
    """The bench step itself: the B = 32 batch of `dist` in `mixed` at the default kernel choices (shared by A and C)."""
    key = "out_" + dist
    if key not in st:
        pipe = _get(st, "pipe")
        pipe.set_precision("mixed")
        st[key] = pipe(*_get(st, dist)[:3])
    return st[key]


def _check_equivariance(pipe, batch, n, out=None):
    """Part A: the batch in its order and reversed -> the same per-scene outputs, bit for bit; returns the forward-order output."""
    pts, off, patches, pts_np, patches_np = batch
    if out is None:
        out = pipe(pts, off, patches)
    rev = pipe(*_batch(pts_np, patches_np, list(range(n))[::-1]))
    assert not torch.equal(out["lidar_tokens"][0], out["lidar_tokens"][n - 1])       # the scenes differ: a permutation is visible
    bad = {i: d for i in range(n) if (d := _diff(out, i, rev, n - 1 - i))}
    assert not bad, f"scene -> outputs that change with its position (first bad scene {min(bad)}): {bad}"
    return out


def _assert_large_offsets(pipe, unsigned_range: bool):
    """Non-vacuity of A: the rows of this batch reach the offsets the test exists for."""
    cfg = pipe.cfg
    hw, d2 = cfg.bev_hw[0] * cfg.bev_hw[1], 2 * cfg.d_model
    dirty = int(pipe.vat_lidar._last_tile_counts[2])
    assert (hw + dirty) * d2 > 2 ** 31, (hw, dirty)
    if unsigned_range:
        assert hw + dirty > 2 ** 32 // d2, (hw, dirty)


# ---- A: position equivariance at the shipped defaults ---------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_bench_batch_reversed_is_the_same_batch(state, mode):
    """The 32 bench scenes and the same scenes reversed: every per-scene output equal bit for bit after the permutation (fused and LiDAR
    tokens, pillar coordinates and features, the 3-D branch's coordinates, counts and features; the batch column = the scene's position).
    A scene that is right at position 0 and wrong at position 31 fails here."""
    pipe = _get(state, "pipe")
    pipe.set_precision(mode)
    if mode == "mixed":
        out = _check_equivariance(pipe, _get(state, "C"), S, _mixed_out(state, "C"))
        _assert_large_offsets(pipe, unsigned_range=False)
    else:
        out = _check_equivariance(pipe, _get(state, "C"), S)
    if mode in ("mixed", "mixed16"):
        assert _tripped(pipe) is None
    assert bool(torch.isfinite(out["fused"]).all())


def test_bench_batch_reversed_dist_u(state):
    """value_dist_u's batch (69 % dirty cells: the unsigned stream, computed rows past 2^32 elements of the K|V buffer) in `mixed`."""
    pipe = _get(state, "pipe")
    pipe.set_precision("mixed")
    out = _mixed_out(state, "U")
    _assert_large_offsets(pipe, unsigned_range=True)
    _check_equivariance(pipe, _get(state, "U"), S, out)
    assert _tripped(pipe) is None


# ---- C: the late scenes against the CPU oracle ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dist", ["C", "U"])
def test_bench_batch_last_scene_meets_the_bar(state, dist):
    """Scene 31 at position 31 of the B = 32 `mixed` step against the CPU oracle at 1e-3 (fused and LiDAR tokens)."""
    from oracle import pipeline_oracle as PO
    pipe = _get(state, "pipe")
    out = _mixed_out(state, dist)
    _, _, _, pts_np, patches_np = _get(state, dist)
    sd = lambda m: {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref = PO.run(_cfg(dist=dist), pts_np[S - 1:S], patches_np[S - 1:S], sd(pipe.pillar_vfe), sd(pipe.vat_lidar), sd(pipe.fuse), do_3d=False)
    err_f = (out["fused"][S - 1].cpu() - ref["fused"][0]).abs().max().item()
    err_l = (out["lidar_tokens"][S - 1].cpu() - ref["lidar_tokens"][0]).abs().max().item()
    print(f"Dist-{dist} scene {S - 1} at position {S - 1}: fused {err_f:.3e}, lidar_tokens {err_l:.3e}")
    assert err_f < TOL and err_l < TOL, (dist, err_f, err_l)


# ---- B: every scene equals itself run alone -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_bench_batch_scene_alone_is_the_scene_in_the_batch(state, mode):
    """With the batch-dependent kernel choices pinned (PINNED), scene i alone (B = 1) and at position i of the 32-scene batch give the same
    outputs bit for bit -- every scene in `mixed`, scenes 0, 15, 16, 31 in the other modes; and the scenes of a 13-scene batch (scenes
    19..31: three groups of four and a remainder of one) likewise.  One module runs B = 1 -> 13 -> 32 -> 1: its K|V buffers (built for the
    first call of the mode) grow twice, then the large ones serve a single scene."""
    from lidar_vision_vqa_amd import _ffi
    pipe = _get(state, "pipe")
    pts, off, patches, pts_np, patches_np = _get(state, "C")
    scenes = list(range(S)) if mode == "mixed" else [0, 15, 16, 31]
    b13 = list(range(S - 13, S))
    h, w = pipe.cfg.bev_hw
    pipe.set_precision(mode)
    tiled = mode != "bf16x3"                     # bf16x3 runs the dense route: no K|V buffers
    for k in _kv_keys(pipe):                     # start from an empty K|V cache, as a module that has seen no batch of this mode yet
        del pipe.vat_lidar._pe_cache[k]
    alone = {}
    with _ffi.tuning(**PINNED):
        first = pipe(*_batch(pts_np, patches_np, [scenes[0]]))
        if tiled:
            assert _kv_rows(pipe) == 2 * h * w
        out13 = pipe(*_batch(pts_np, patches_np, b13))
        if tiled:
            assert _kv_rows(pipe) == 14 * h * w
        out32 = pipe(pts, off, patches)
        if tiled:
            assert _kv_rows(pipe) == 33 * h * w
        for i in scenes:
            alone[i] = pipe(*_batch(pts_np, patches_np, [i]))
        if tiled:
            assert _kv_rows(pipe) == 33 * h * w
    assert not _diff(first, 0, alone[scenes[0]], 0), "B = 1 on the grown K|V buffers differs from B = 1 on the first ones"
    bad = {i: d for i in scenes if (d := _diff(alone[i], 0, out32, i))}
    assert not bad, f"{mode}: scene -> outputs that differ between B = 1 and B = 32 (first bad scene {min(bad) if bad else None}): {bad}"
    bad13 = {i: d for i in scenes if i in b13 and (d := _diff(alone[i], 0, out13, b13.index(i)))}
    assert not bad13, f"{mode}: scene -> outputs that differ between B = 1 and B = 13: {bad13}"
    if mode in ("mixed", "mixed16"):
        assert _tripped(pipe) is None


# ---- value_n_layers_4: A and B on its B = 8 batch -------------------------------------------------------------------------------------

def test_bench_batch_n_layers_4(state):
    """VATLiDAR(n_layers = 4) on the bench's 8 scenes in `mixed` (blocks 1..3 stream every key of every scene through the unsigned tiled
    kernel): the batch reversed is the same batch (default choices), and every scene alone equals itself in the batch (PINNED)."""
    from lidar_vision_vqa_amd import _ffi
    pipe = _get(state, "pipe4")
    batch = _get(state, "L4")
    _check_equivariance(pipe, batch, 8)
    assert _tripped(pipe) is None
    pts, off, patches, pts_np, patches_np = batch
    with _ffi.tuning(**PINNED):
        out8 = pipe(pts, off, patches)
        bad = {i: d for i in range(8) if (d := _diff(pipe(*_batch(pts_np, patches_np, [i])), 0, out8, i))}
    assert not bad, f"L = 4: scene -> outputs that differ between B = 1 and B = 8: {bad}"
    assert _tripped(pipe) is None
    del state["pipe4"], state["L4"]
    gc.collect()
    torch.cuda.empty_cache()


# ---- D: dense-canvas input at the bench's size ----------------------------------------------------------------------------------------

def test_bench_batch_dense_canvas_input(state):
    """value_dense_canvas_input: PointPillarScatter's [8, 64, 512, 512] canvas -> VATLiDAR.forward(bev) (lvq_bev_occupied_cells turns it
    back into pillars) gives the sparse pipeline's LiDAR and fused tokens bit for bit on the bench's 8-scene batch."""
    from lidar_vision_vqa_amd import pipeline as P
    sparse = _get(state, "pipe")
    sparse.set_precision("mixed")
    dense = P.FusionPipeline(_cfg(), DEV, precision="mixed", dense_bev=True)
    dense.load_state_dict(sparse.state_dict())
    pts, off, patches, pts_np, patches_np = _get(state, "C")
    b8 = _batch(pts_np, patches_np, range(8))
    a, b = sparse(*b8), dense(*b8)
    assert a["bev"] is None and tuple(b["bev"].shape) == (8, 64) + sparse.cfg.bev_hw
    assert torch.equal(a["lidar_tokens"], b["lidar_tokens"])
    assert torch.equal(a["fused"], b["fused"])
    assert _tripped(sparse) is None and _tripped(dense) is None
