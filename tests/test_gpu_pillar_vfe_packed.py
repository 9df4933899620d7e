"""k_pillar_vfe_packed (csrc/vfe.hip: lvq_tuning.pillar_vfe_path = 0, the default single-layer PillarVFE kernel) against k_pillar_vfe1
(pillar_vfe_path = 1), through the C ABI.  The packed kernel runs the prologue for two pillars per wave pass, stages only the live
points' feature rows -- rows of several pillars back to back -- into 16-row LDS tiles and multiplies them on v_mfma_f32_16x16x4_f32;
it must return the bits of the one-pillar-per-wave kernel.  A wave owns 16 consecutive pillars (8 passes), a workgroup 64.

Every output buffer is larger than the result and pre-filled: rows at and behind the live count, and the tail, must keep the pattern."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lidar_feature_cases as LF  # noqa: E402
from lidar_vision_vqa_amd import _ffi as F  # noqa: E402

DEV = "cuda:0"
FILL = -7.25
TAIL = 5                                                                        # rows allocated behind m_cap
PACKED, ONE_PER_WAVE = 0, 1                                                     # lvq_tuning.pillar_vfe_path


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def run(k, misalign=False):
    """The live rows of a case (the keys of LF.pillar_case) under the tuning record in force; the rows behind the live count and the
    tail must keep the pattern."""
    cap, m, t, c = k["cap"], k["m"], k["t"], k["c"]
    if misalign:                                                                # voxels 4 bytes off a 16-byte line
        buf = torch.zeros((cap * t * c + 1,), dtype=torch.float32, device=DEV)
        vox = buf[1:]
        vox.copy_(dev(k["voxels"]).reshape(-1))
        assert vox.data_ptr() % 16 == 4
    else:
        vox = dev(k["voxels"])
        assert vox.data_ptr() % 16 == 0
    w, sc, sh = (dev(a, np.float32) for a in k["layers"][0])
    cout, cin = k["layers"][0][0].shape
    out = torch.full((cap + TAIL, cout), FILL, dtype=torch.float32, device=DEV)
    num, coords, n_dev = dev(k["num"]), dev(k["coords"]), dev(np.array([m], np.int32))
    rc = F.lib().lvq_pillar_vfe(F.ptr(vox), F.ptr(num), F.ptr(coords), F.i64(cap), F.ptr(n_dev), F.cint(t), F.cint(c), F.cint(1),
                                F.ptr_array([w]), F.ptr_array([sc]), F.ptr_array([sh]), F.i32x([cin]), F.i32x([cout]), F.cint(k["flags"]),
                                F.f32x(LF.VS.tolist()), F.f32x(LF.OFF.tolist()), F.ptr(out), F.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0, F.lib().lvq_strerror(rc)
    got = out.cpu().numpy()
    assert (got[m:] == FILL).all(), "rows behind n_voxels_dev, or the tail, were written"
    return got[:m]


def both_paths(tune, k):
    tune(pillar_vfe_generic=0, pillar_vfe_path=PACKED)
    packed = run(k)
    tune(pillar_vfe_path=ONE_PER_WAVE)
    one = run(k)
    tune(pillar_vfe_path=PACKED)
    return packed, one


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the existing case list
# ---------------------------------------------------------------------------------------------------------------------------
def test_packed_equals_one_per_wave_on_the_single_layer_cases(tune):
    """Every case of LF.pillar_single_layer_cases(): the two paths return the same bits, and the result lies within 2 x the case's own
    first-order fp32 bound of its fp64 reference."""
    worst = 0.0
    for args in LF.pillar_single_layer_cases():
        k = LF.pillar_case(*args)
        packed, one = both_paths(tune, k)
        assert same_bits(packed, one), (args, int((packed != one).sum()))
        err = np.abs(packed.astype(np.float64) - k["ref"])
        assert (err <= 2.0 * k["bound"]).all(), (args, float((err / k["bound"]).max()))
        worst = max(worst, float((err / k["bound"]).max()))
    print(f"k_pillar_vfe_packed, single-layer cases: largest err/bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. packing boundaries
# ---------------------------------------------------------------------------------------------------------------------------
def custom_case(nums, t, cout, flags, seed, m=None, extra=13, zero=False):
    """len(nums) pillars with the given num_points (the first m of them live; `extra` more rows of ordinary pillars behind them, which
    a kernel that ran them would write).  Channel 0 is LF.pillar_case's pad probe: it reads the non-negative intensity alone with a
    negative weight and a positive shift, so relu(shift) is its maximum wherever a padded slot takes part."""
    rng = np.random.default_rng(seed)
    nums = list(nums)
    m = len(nums) if m is None else m
    num = np.array(nums + [(1, 2, t - 1, t)[i % 4] for i in range(extra)], np.int32)
    num = np.maximum(num, 1)
    cap = len(num)
    cells = np.stack([rng.integers(0, LF.GRID[0], cap), rng.integers(0, LF.GRID[1], cap), rng.integers(0, LF.GRID[2], cap)], axis=1)
    coords = np.stack([rng.integers(0, 2, cap), cells[:, 2], cells[:, 1], cells[:, 0]], axis=1).astype(np.int32)
    vox = LF.cell_points(rng, np.repeat(cells[:, None, :], t, axis=1), 4)
    vox[np.arange(t)[None, :] >= num[:, None]] = 0.0                            # the voxeliser leaves padding slots zero
    if zero:
        vox[:] = 0.0
    layers = LF.pfn_params(LF.pfn_cin(4, flags), (cout,), seed + 1, True)
    layers[0][0][0, :] = 0.0
    layers[0][0][0, 3 if flags & 1 else 0] = -0.7
    layers[0][2][0] = 0.3
    return dict(voxels=vox, num=num, coords=coords, m=m, cap=cap, t=t, c=4, layers=layers, flags=flags)


T32 = 32
# num_points lists (T = 32): live-row totals 1, 15, 16, 17, 31, 32, 33; a pillar across a tile boundary; two full tiles between single
# points; last tiles of one row; a pass of 64 rows onto 15 waiting ones (the ring's largest fill); a count above T (clamped to T slots)
BOUNDARY_NUMS = {
    "total1": [1], "total15": [7, 8], "total16": [7, 9], "total16_one_pillar": [16], "total17_last_tile_one_row": [7, 9, 1],
    "total31": [20, 11], "total32": [20, 12], "total33": [20, 12, 1],
    "straddle": [10, 10, 10], "full_between_singles": [1, 32, 1], "two_full_then_one": [32, 32, 1],
    "ring_15_plus_64": [8, 7, 32, 32, 1, 1, 30, 3], "all_full_group": [32] * 16 + [1], "all_single": [1] * 35,
    "count_above_T": [1, 35, 2],
}


@pytest.mark.parametrize("cout,flags", list(itertools.product(LF.FAST_COUT, LF.FLAGS)))
def test_packing_boundaries(tune, cout, flags):
    """Bit identity with k_pillar_vfe1 at the row totals and pillar layouts where the tile packing takes another route, for every
    cout in {8, 48, 64} x flags; channel 0 holds the pad value exactly where num_points < T and stays below it where num_points >= T."""
    for i, (name, nums) in enumerate(BOUNDARY_NUMS.items()):
        k = custom_case(nums, T32, cout, flags, 8100 + 16 * i + flags)
        packed, one = both_paths(tune, k)
        assert same_bits(packed, one), (name, cout, flags)
        sc0, sh0 = k["layers"][0][1][0], k["layers"][0][2][0]
        pad = max(np.float32(np.float32(0.0) * sc0) + sh0, np.float32(0.0))
        padded = k["num"][:k["m"]] < T32
        assert (packed[padded, 0] == pad).all(), (name, "the padded-slot value is missing")
        assert (packed[~padded, 0] < pad).all(), (name, "a padded-slot value entered a full pillar")


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 33, 257])
def test_live_count_cuts_a_pass_and_a_group(tune, m):
    """M live pillars of T = 20 in a larger buffer: an odd M ends inside a pass of two, 33 and 257 one pillar into a wave's group of 16 and
    a workgroup's 64.  Behind the live count lie 13 ordinary pillars, or a single one (the other half of the last pass, or the first
    pillar of a group whose wave must leave at once): none of them may be written."""
    nums = [(1, 2, 19, 20, 3, 1, 1, 20)[i % 8] for i in range(m)]
    for extra in (13, 1):
        k = custom_case(nums, 20, 64, 1 + 2 * (m & 1), 8600 + m, extra=extra)
        packed, one = both_paths(tune, k)
        assert same_bits(packed, one), (m, extra)


@pytest.mark.parametrize("flags", LF.FLAGS)
def test_all_zero_points(tune, flags):
    """Every point (0, 0, 0, 0): products of both signs of zero, and at cin = 10 no padded k position; the accumulators' zero signs must
    not reach an output bit."""
    for cout in LF.FAST_COUT:
        k = custom_case([1, 2, 19, 20, 20, 7, 1], 20, cout, flags, 8700 + flags, zero=True)
        packed, one = both_paths(tune, k)
        assert same_bits(packed, one), (cout, flags)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. one real distribution
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", ["C", "U"])
def test_one_scene_through_the_pipelines_voxeliser(tune, dist):
    """The pillars of one 32 768-point scene (the pipeline's pillar voxeliser: 0.2 m, T = 20, and its PillarVFE[64] with the pipeline's
    seeded weights): the two paths agree bit for bit.  Prints the pillar count and the live points per pillar."""
    from lidar_vision_vqa_amd import lidar, synth
    from lidar_vision_vqa_amd.pipeline import Cfg, PipelineConfig
    cfg = PipelineConfig(dist=dist)
    rng = list(cfg.pc_range)
    gen = lidar.VoxelGeneratorWrapper(cfg.voxel_pillar, rng, 4, cfg.t_pillar, cfg.max_pillars)
    vfe = lidar.PillarVFE(Cfg(USE_NORM=True, WITH_DISTANCE=False, USE_ABSLOTE_XYZ=True, NUM_FILTERS=cfg.pillar_filters), 4,
                          list(cfg.voxel_pillar), rng)
    synth.load_seeded(vfe, cfg.weight_seed)
    vfe = vfe.to(DEV).eval()
    pts = torch.from_numpy(synth.scene_points(dist, cfg.n_points, 1001)).to(DEV)
    off = torch.tensor([0, pts.shape[0]], dtype=torch.int32, device=DEV)
    vox, coords, num, svo = gen.generate_batch_device(pts, off, 1)
    m = int(svo[1].item())
    live = torch.clamp(num[:m], max=cfg.t_pillar)
    print(f"Dist-{dist}: {pts.shape[0]} points -> {m} pillars, {int(live.sum())} live points, {float(live.float().mean()):.3f} per pillar, "
          f"largest {int(live.max())}, {int((num[:m] == 1).sum())} pillars of one point")
    res = {}
    for path in (PACKED, ONE_PER_WAVE):
        tune(pillar_vfe_generic=0, pillar_vfe_path=path)
        got = vfe.forward_device(vox, num, coords, svo[1:])
        torch.cuda.synchronize()
        res[path] = got[:m].cpu().numpy()
    assert np.isfinite(res[PACKED]).all()
    assert same_bits(res[PACKED], res[ONE_PER_WAVE]), int((res[PACKED] != res[ONE_PER_WAVE]).sum())


# ---------------------------------------------------------------------------------------------------------------------------
# 4. misaligned voxels
# ---------------------------------------------------------------------------------------------------------------------------
def test_misaligned_voxels_still_take_the_generic_kernel(tune):
    """voxels 4 bytes off a 16-byte line: neither single-layer kernel may run (both load float4); the bits are k_pillar_vfe<32>'s under
    either pillar_vfe_path."""
    for flags in (1, 3):
        k = LF.pillar_case(33, 20, 4, (64,), flags, 7950 + flags, True)
        tune(pillar_vfe_generic=1, pillar_vfe_path=PACKED)
        generic = run(k)
        err = np.abs(generic.astype(np.float64) - k["ref"])
        assert (err <= 2.0 * k["bound"]).all()
        for path in (PACKED, ONE_PER_WAVE):
            tune(pillar_vfe_generic=0, pillar_vfe_path=path)
            assert same_bits(run(k, misalign=True), generic), f"a misaligned voxel pointer must run k_pillar_vfe<32> (pillar_vfe_path = {path})"
