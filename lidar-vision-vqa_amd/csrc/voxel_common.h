// csrc/voxel_common.h -- what the three voxeliser files (voxel.hip, voxel_binned.hip, voxel_hashed.hip) share: the grid geometry and the
// cell rule, the small device helpers (scene lookup, prefix popcount, wave / block scans, reciprocal integer division), the first-rank
// rule of the two paths that rank first points by a flag-word prefix, and the internal entry points through which voxel.hip reaches
// the other two files.  Included by those three files only.
#pragma once
#include "common.h"

// -------------------------------------------------------------------------------------------------
// internal ABI: the slab paths behind lvq_voxelize_hard / lvq_voxelize_mean / lvq_voxelize_dynamic (voxel.hip validates the arguments
// and the workspace size first).  They return LVQ_EUNSUPPORTED for shapes they do not take and the caller tries the next path.
// -------------------------------------------------------------------------------------------------
// key-contiguous slabs (voxel_binned.hip)
size_t lvq_binned_dynamic_workspace_bytes(int64_t n);
int lvq_binned_voxelize_dynamic(const float *pts, int64_t n, int c, int batch_size, const float *range_host,
                                const float *vsize_host, const int32_t *grid_host, int ndim, int32_t *unq_inv, int32_t *pt_coords,
                                int32_t *unq_key, int32_t *unq_cnt, int32_t *coords_bzyx, int32_t *counts, void *ws, size_t ws_bytes,
                                hipStream_t st);
size_t lvq_binned_hard_workspace_bytes(int64_t n, int n_scenes);
int lvq_binned_voxelize_hard(const float *pts, const int32_t *scene_off, int64_t n, int n_scenes, int c, const float *range_host,
                             const float *vsize_host, const int32_t *grid_host, int max_pts, int max_voxels, float *voxels,
                             int32_t *coords_bzyx, int32_t *num_pts, int32_t *scene_voxel_off, void *ws, size_t ws_bytes,
                             hipStream_t st);
// hash-balanced slabs + input-order placement (voxel_hashed.hip): the default hard path, and the only fused voxelise -> mean one
size_t lvq_hashed_hard_workspace_bytes(int64_t n, int n_scenes);
int lvq_hashed_voxelize_hard(const float *pts, const int32_t *scene_off, int64_t n, int n_scenes, int c, const float *range_host,
                             const float *vsize_host, const int32_t *grid_host, int max_pts, int max_voxels, float *voxels,
                             int32_t *coords_bzyx, int32_t *num_pts, int32_t *scene_voxel_off, void *ws, size_t ws_bytes,
                             hipStream_t st);
int lvq_hashed_voxelize_mean(const float *pts, const int32_t *scene_off, int64_t n, int n_scenes, int c, const float *range_host,
                             const float *vsize_host, const int32_t *grid_host, int max_pts, int max_voxels, float *voxel_features,
                             int32_t *coords_bzyx, int32_t *num_pts, int32_t *scene_voxel_off, void *ws, size_t ws_bytes,
                             hipStream_t st);

// -------------------------------------------------------------------------------------------------
// geometry and the cell rule
// -------------------------------------------------------------------------------------------------
struct Geom {
    float lo[3];
    float vs[3];
    int grid[3];
};

static inline Geom make_geom(const float *range_host, const float *vsize_host, const int32_t *grid_host) {
    Geom g;
    for (int j = 0; j < 3; ++j) { g.lo[j] = range_host[j]; g.vs[j] = vsize_host[j]; g.grid[j] = grid_host[j]; }
    return g;
}

// cell coordinates (cx, cy, cz) of a point: floor((p - lo) / vs) in IEEE fp32 over the first ndim axes, in-range test on the float as
// the reference does it.  An axis outside the grid gets -1 and the result is false; axes >= ndim stay 0.  This is THE rule the project
// promises bit for bit: subtract, divide, floor, compare as float, cast -- in that order.
__device__ __forceinline__ bool cell_of(const float xyz[3], const Geom &g, int ndim, int cc[3]) {
    bool ok = true;
    cc[0] = cc[1] = cc[2] = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j < ndim) {
            float d = xyz[j] - g.lo[j];
            float q = d / g.vs[j];
            float f = floorf(q);
            bool in = (f >= 0.0f) && (f < (float)g.grid[j]);  // NaN/inf fail here like (int) casts do on the CPU
            ok = ok && in;
            cc[j] = in ? (int)f : -1;
        }
    }
    return ok;
}

// scene of point i: the largest s with off[s] <= i
__device__ __forceinline__ int find_scene(const int32_t *off, int n_scenes, int i) {
    int lo = 0, hi = n_scenes;
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// set bits of m below position `bit` (0..63)
__device__ __forceinline__ int popc_below(uint64_t m, int bit) {
    return __popcll(m & ((bit == 0) ? 0ull : (~0ull >> (64 - bit))));
}

// -------------------------------------------------------------------------------------------------
// scans
// -------------------------------------------------------------------------------------------------
// inclusive scan of one int per lane over the wave (lane = threadIdx.x & 63)
__device__ __forceinline__ int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    return incl;
}

// block-wide exclusive scan of one int per thread; wave_tot holds nwaves ints of LDS.  nwaves MUST equal blockDim.x / 64 (it is not
// derived from blockDim: pass the launch size's compile-time constant, so the loop over the wave totals unrolls).  Two barriers:
// wave_tot may be reused as soon as the call returns.  The wave index is compared as a thread index (threadIdx.x >= 64 (w + 1)) and
// only formed for the store: a kernel with several scans then keeps no wave-index register alive between them.
__device__ __forceinline__ int block_excl_scan(int v, int *wave_tot, int nwaves, int &total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int incl = wave_incl_scan(v);
    if (lane == 63) wave_tot[wid] = incl;
    __syncthreads();
    int wbase = 0, tot = 0;
    for (int w = 0; w < nwaves; ++w) {
        const int t = wave_tot[w];
        if ((int)threadIdx.x >= 64 * (w + 1)) wbase += t;   // w < wave index
        tot += t;
    }
    __syncthreads();
    total = tot;
    return wbase + incl - v;
}

// -------------------------------------------------------------------------------------------------
// floor(a / d) through the fp32 reciprocal rd = 1.0f / (float)d, d >= 1
// -------------------------------------------------------------------------------------------------
// 0 <= a < 2^31.  The fp32 estimate is within a few units of the quotient (relative error 2^-23 of a quotient < 2^26); the correction
// LOOPS make it exact for every a.  (A single correction step each way is NOT enough here: above ~2^29 the estimate is off by more than
// one divisor and keys of scenes >= 12 on the 0.1 m grid decoded to wrong (z, y, x) -- found by
// tests/test_gpu_lidar.py::test_hard_voxelizer_paths_agree_at_scale.)
__device__ __forceinline__ int idiv_rcp(int a, int d, float rd) {
    int q = (int)((float)a * rd);
    int r = a - q * d;
    while (r < 0) { --q; r += d; }
    while (r >= d) { ++q; r -= d; }
    return q;
}

// 0 <= a < 2^23 ONLY: (float)a is exact and the estimate is within one of the quotient, so one correction step each way is enough.
// For store loops over small indices; anything that decodes a key uses idiv_rcp.
__device__ __forceinline__ int idiv_rcp_small(int a, int d, float rd) {
    int q = (int)((float)a * rd);
    int r = a - q * d;
    if (r < 0) { --q; r += d; }
    if (r >= d) ++q;
    return q;
}

// -------------------------------------------------------------------------------------------------
// first-appearance ranks from a flag-word prefix (voxel.hip's global-hash path and voxel_binned.hip's hard path)
// -------------------------------------------------------------------------------------------------
// number of first points with an index below i: fmask = 1 bit per point, wpre = exclusive popcount prefix of its words
__device__ __forceinline__ int first_rank(const uint64_t *fmask, const int32_t *wpre, int i) {
    return wpre[i >> 6] + popc_below(fmask[i >> 6], i & 63);
}

// Scene offsets of those two paths, one single-workgroup kernel (k_hard_scene_offsets, voxel.hip): sfr[s] = first-rank at the start of
// scene s (s = 0..n_scenes), scene_voxel_off = packed output offsets under the max_voxels cap; nwords = words of fmask that hold flags.
void lvq_hard_scene_offsets(const int32_t *scene_off, int n_scenes, int nwords, int max_voxels, const uint64_t *fmask,
                            const int32_t *wpre, int32_t *sfr, int32_t *scene_voxel_off, hipStream_t st);
