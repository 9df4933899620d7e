// csrc/sparse_conv.hip -- the sparse convolutions of VoxelResBackBone8xVoxelNeXt, VoxelBackBone8x / VoxelResBackBone8x and PillarBackBone8x /
// PillarRes18BackBone8x (spconv 2.x SubMConv3d / SparseConv3d / SparseConv2d / SubMConv2d as pcdet/models/backbones_3d/
// spconv_backbone_voxelnext.py:8-225, spconv_backbone.py:8-295 and spconv_backbone_2d.py:8-300 use them), gfx950.
//
//   lvq_sparse_conv_rules   the active output set and the neighbour table nbr [n_out, K] (input row per kernel offset, -1 = absent).
//                           No hash table and no sort: the ascending-unique machinery of the dynamic voxeliser (voxel.hip /
//                           voxel_binned.hip) ranks integer cells exactly as it ranks points, as lvq_sparse_bev_merge already does.
//                             regular conv: every input row proposes the output sites it reaches (prod ceil(k / s) candidates: 8 for
//                               kernel 3 stride 2, 9 / 27 for stride 1); the voxeliser returns the unique sites in ascending (b, z, y, x)
//                               order and the rank of every candidate, which IS its row of the table: nbr[rank][offset] = input row
//                               (one writer per entry: an (output site, offset) pair has one input cell).
//                             submanifold: the inputs themselves are ranked; a neighbour is found by a binary search over the ascending
//                               keys (32 steps at most), then rank -> input row.
//                           Every axis is range-checked before a key is formed, so a neighbour across an x / y / z / scene edge is absent.
//   lvq_sparse_conv         gather-form implicit GEMM: one workgroup = 64 output rows x all C_out; its four waves split the columns first
//                           (16 / 32 per wave for C_out 64 / 128: a W_o fragment is then read once per workgroup), the rows otherwise.  Per kernel
//                           offset, in ascending order: the tile's neighbour rows are gathered (coalesced fp32 row reads) into LDS as
//                           bf16 hi (+ lo), each wave multiplies its rows with its columns of W_o [C_out, C_in] on v_mfma_f32_16x16x32_bf16 tiles
//                           (fp32 accumulators; hi*hi + hi*lo + lo*hi in the bf16x3 form) and the folded BatchNorm / ReLU / residual
//                           epilogue is applied from the accumulators.  An offset no row of the tile has is skipped (a row without it
//                           adds exact zeros, so skipping changes no bit): a row's result depends on its own neighbours only.
//                           C_in of 4 / 5 / 16 is zero-padded to the MFMA depth of 32 in LDS and in the packed weights.
//                           C_out = 256 (C_in 128 or 256): a wave owns 64 columns; C_in = 256 runs as two 128-channel stages per offset,
//                           ascending, each with its own gather and its own weight fragments, so LDS stays that of the 128-channel tile.
#include "common.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

namespace {

constexpr int MAXK = 27;

struct RuleGeom {
    int ndim, batch, subm;
    int in[3], out[3], k[3], s[3], p[3];      // (z, y, x); 2-D problems use in[0] = out[0] = k[0] = s[0] = 1, p[0] = 0
    int kc[3];                                // candidates per axis: ceil(k / s)
    int kvol, kcand;
};

// an index row -> (b, z, y, x); false when it lies outside the grid or the batch
__device__ __forceinline__ bool load_cell(const int32_t *__restrict__ idx, int64_t i, const RuleGeom &g, int &b, int c[3]) {
    const int32_t *row = idx + i * (g.ndim + 1);
    b = row[0];
    c[0] = g.ndim == 3 ? row[1] : 0;
    c[1] = row[g.ndim - 1];
    c[2] = row[g.ndim];
    return b >= 0 && b < g.batch && c[0] >= 0 && c[0] < g.in[0] && c[1] >= 0 && c[1] < g.in[1] && c[2] >= 0 && c[2] < g.in[2];
}

// candidate j of input cell c: the j-th kernel offset (per axis) that lands on an output site; returns the offset index or -1
__device__ __forceinline__ int candidate(const RuleGeom &g, const int c[3], int j, int q[3]) {
    int o[3];
    int jj = j;
    bool ok = true;
#pragma unroll
    for (int a = 2; a >= 0; --a) {
        const int ja = jj % g.kc[a];
        jj /= g.kc[a];
        const int t = c[a] + g.p[a];                       // q * s + o = c + p
        o[a] = t % g.s[a] + ja * g.s[a];
        const int num = t - o[a];
        q[a] = num / g.s[a];
        ok = ok && o[a] < g.k[a] && num >= 0 && q[a] < g.out[a];
    }
    return ok ? (o[0] * g.k[1] + o[1]) * g.k[2] + o[2] : -1;
}

__device__ __forceinline__ float4 cell_point(const RuleGeom &g, int b, const int q[3]) {
    return g.ndim == 3 ? make_float4((float)b, (float)q[0], (float)q[1], (float)q[2]) : make_float4((float)b, (float)q[1], (float)q[2], 0.f);
}

__global__ void __launch_bounds__(256) k_rules_cand(const int32_t *__restrict__ idx, int64_t n, RuleGeom g, float4 *__restrict__ pts) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * g.kcand) return;
    const int64_t i = t / g.kcand;
    const int j = (int)(t - i * g.kcand);
    int b, c[3], q[3];
    float4 p = make_float4(-1.f, -1.f, -1.f, -1.f);           // outside every grid: the voxeliser drops it (unq_inv = -1)
    if (load_cell(idx, i, g, b, c) && candidate(g, c, j, q) >= 0) p = cell_point(g, b, q);
    pts[t] = p;
}

__global__ void __launch_bounds__(256) k_subm_pts(const int32_t *__restrict__ idx, int64_t n, RuleGeom g, float4 *__restrict__ pts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int b, c[3];
    pts[i] = load_cell(idx, i, g, b, c) ? cell_point(g, b, c) : make_float4(-1.f, -1.f, -1.f, -1.f);
}

__device__ __forceinline__ int64_t live_rows(const int32_t *__restrict__ counts, int64_t cap) {
    int64_t m = counts[0];
    return m < 0 ? 0 : (m > cap ? cap : m);
}

// rows [0, n_out) of the table = -1; the output index rows from the ascending keys; the row count
__global__ void __launch_bounds__(256) k_rules_out(const int32_t *__restrict__ unq_key, const int32_t *__restrict__ counts, int64_t cap, RuleGeom g,
                                                   int32_t *__restrict__ out_idx, int32_t *__restrict__ nbr, int32_t *__restrict__ n_out) {
    const int64_t m = live_rows(counts, cap);
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t == 0) *n_out = counts[0];
    if (t < m * g.kvol) nbr[t] = -1;
    if (t < m) {
        int64_t key = unq_key[t];
        const int x = (int)(key % g.out[2]); key /= g.out[2];
        const int y = (int)(key % g.out[1]); key /= g.out[1];
        int32_t *row = out_idx + t * (g.ndim + 1);
        if (g.ndim == 3) {
            row[0] = (int)(key / g.out[0]); row[1] = (int)(key % g.out[0]); row[2] = y; row[3] = x;
        } else {
            row[0] = (int)key; row[1] = y; row[2] = x;
        }
    }
}

__global__ void __launch_bounds__(256) k_rules_scatter(const int32_t *__restrict__ idx, int64_t n, RuleGeom g, const int32_t *__restrict__ unq_inv,
                                                       const int32_t *__restrict__ counts, int64_t cap, int32_t *__restrict__ nbr) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * g.kcand) return;
    const int64_t r = unq_inv[t];
    if (r < 0 || r >= live_rows(counts, cap)) return;
    const int64_t i = t / g.kcand;
    int b, c[3], q[3];
    if (!load_cell(idx, i, g, b, c)) return;
    const int o = candidate(g, c, (int)(t - i * g.kcand), q);
    if (o >= 0) nbr[r * g.kvol + o] = (int32_t)i;
}

__global__ void __launch_bounds__(256) k_subm_rowof(const int32_t *__restrict__ unq_inv, int64_t n, int32_t *__restrict__ rowof, int32_t *__restrict__ n_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *n_out = (int32_t)n;
    if (i >= n) return;
    const int r = unq_inv[i];
    if (r >= 0 && r < n) rowof[r] = (int32_t)i;
}

__global__ void __launch_bounds__(256) k_subm_nbr(const int32_t *__restrict__ idx, int64_t n, RuleGeom g, const int32_t *__restrict__ unq_key,
                                                  const int32_t *__restrict__ counts, const int32_t *__restrict__ rowof, int32_t *__restrict__ nbr) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * g.kvol) return;
    const int64_t i = t / g.kvol;
    const int o = (int)(t - i * g.kvol);
    int b, c[3];
    int res = -1;
    if (load_cell(idx, i, g, b, c)) {
        const int oz = o / (g.k[1] * g.k[2]), oy = (o / g.k[2]) % g.k[1], ox = o % g.k[2];
        const int z = c[0] + oz - g.k[0] / 2, y = c[1] + oy - g.k[1] / 2, x = c[2] + ox - g.k[2] / 2;
        if (z >= 0 && z < g.in[0] && y >= 0 && y < g.in[1] && x >= 0 && x < g.in[2]) {
            const int64_t key = (((int64_t)b * g.in[0] + z) * g.in[1] + y) * g.in[2] + x;      // < 2^31 (checked on the host)
            int lo = 0, hi = (int)live_rows(counts, n);
            for (int it = 0; it < 32 && lo < hi; ++it) {       // first rank with unq_key >= key
                const int mid = (int)(((int64_t)lo + hi) >> 1);
                if ((int64_t)unq_key[mid] < key) lo = mid + 1; else hi = mid;
            }
            if (lo < (int)live_rows(counts, n) && (int64_t)unq_key[lo] == key) res = rowof[lo];
        }
    }
    nbr[t] = res;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// weights [C_out, K, C_in] fp32 -> [K][C_out][cin_pad] bf16 hi (+ lo), zero beyond C_in
__global__ void __launch_bounds__(256) k_pack_w(const float *__restrict__ w, int c_out, int kvol, int c_in, int cin_pad, lvq_bf16 *__restrict__ hi,
                                                lvq_bf16 *__restrict__ lo) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)kvol * c_out * cin_pad) return;
    const int ci = (int)(t % cin_pad);
    const int co = (int)((t / cin_pad) % c_out);
    const int o = (int)(t / ((int64_t)cin_pad * c_out));
    const float v = ci < c_in ? w[((int64_t)co * kvol + o) * c_in + ci] : 0.f;
    const uint16_t h = f32_to_bf16(v);
    hi[t] = h;
    if (lo) lo[t] = f32_to_bf16(v - bf16_to_f32(h));
}

constexpr int TILE_M = 64;

// (C_out = 256 asks for two waves per SIMD: left alone the hi + lo form takes 200 VGPRs + 64 AGPRs, eight over what two workgroups per CU
// allow, and one workgroup per CU has nobody to hide its gather behind; the narrower instantiations keep the compiler's own choice)
template <int CIN_PAD, int COUT, bool SPLIT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(COUT == 256 ? 2 : 1)))
k_sparse_conv(const float *__restrict__ feat, int64_t n_in, int c_in, const int32_t *__restrict__ nbr, int kvol, int64_t n_cap,
              const int32_t *__restrict__ n_out_dev, const lvq_bf16 *__restrict__ w_hi, const lvq_bf16 *__restrict__ w_lo,
              const float *__restrict__ bias, const float *__restrict__ scale, const float *__restrict__ shift,
              const float *__restrict__ residual, int relu, float *__restrict__ out) {
    // K runs in stages of CK channels (one stage up to 128 channels, two for 256): the LDS tile and the weight fragments a wave holds are
    // those of one stage, so C_in = 256 costs no more LDS or registers per column than 128 does
    constexpr int CK = CIN_PAD < 128 ? CIN_PAD : 128, NCH = CIN_PAD / CK;
    constexpr int PITCH = CK + 8;                           // bf16 elements; rows stay 16-byte aligned
    // the four waves as WM x WN: a wave owns MT 16-row tiles x NT 16-column tiles, so a W_o fragment is read once per workgroup (by the
    // one wave that owns its columns) when C_out >= 64, and the LDS rows are read by WN waves
    constexpr int WN = COUT / 16 < 4 ? COUT / 16 : 4, WM = 4 / WN;
    constexpr int MT = TILE_M / 16 / WM, NT = COUT / 16 / WN, KS = CK / 32;
    __shared__ __attribute__((aligned(16))) uint16_t a_hi[TILE_M * PITCH];
    __shared__ __attribute__((aligned(16))) uint16_t a_lo[SPLIT ? TILE_M * PITCH : 8];
    __shared__ int s_nb2[2][TILE_M];                        // by offset parity: wave 0 may post the next offset while others still read this one

    int64_t n_out = n_cap;
    if (n_out_dev) {
        const int64_t v = *n_out_dev;
        n_out = v < 0 ? 0 : (v < n_cap ? v : n_cap);
    }
    const int64_t tile0 = (int64_t)blockIdx.x * TILE_M;
    if (tile0 >= n_out) return;                             // (workgroup-uniform)
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int wm = wid / WN, wn = wid % WN;
    const int row0 = wm * MT * 16, col0 = wn * NT * 16;     // of this wave, inside the tile

    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int o = 0; o < kvol; ++o) {
        int *s_nb = s_nb2[o & 1];
        int r = -1;
        if (tid < TILE_M && tile0 + tid < n_out) {
            r = nbr[(tile0 + tid) * kvol + o];
            if (r < 0 || r >= n_in) r = -1;
        }
        if (tid < TILE_M) s_nb[tid] = r;
        if (!__syncthreads_or(r >= 0)) continue;            // no row of the tile has this offset (uniform; also fences the LDS tile)
#pragma unroll
        for (int kc = 0; kc < NCH; ++kc) {
            if (kc) __syncthreads();                            // the previous stage's LDS tile has been read
            // this wave's W_o fragments of the stage (16 bytes per lane each): issued before the gather, whose latency they share
            bf16x8 bh[KS][NT], bl[KS][NT];
            {
                const int64_t wofs = ((int64_t)o * COUT + col0 + l15) * CIN_PAD + kc * CK + 8 * lq;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        bh[ks][nt] = *reinterpret_cast<const bf16x8 *>(w_hi + wofs + (int64_t)nt * 16 * CIN_PAD + ks * 32);
                        bl[ks][nt] = SPLIT ? *reinterpret_cast<const bf16x8 *>(w_lo + wofs + (int64_t)nt * 16 * CIN_PAD + ks * 32) : bh[ks][nt];
                    }
            }
            // gather: four channels per thread and step, a row's channels on consecutive lanes
            constexpr int QPR = CK / 4;
#pragma unroll
            for (int e0 = 0; e0 < TILE_M * QPR; e0 += 256) {
                const int e = e0 + tid;
                const int row = e / QPR, c4 = (e % QPR) * 4, cg = kc * CK + c4;      // c4: column of the LDS stage, cg: channel of the row
                const int src = s_nb[row];
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (src >= 0 && cg < c_in) {
                    const float *p = feat + (int64_t)src * c_in + cg;
                    if ((c_in & 3) == 0) {
                        const float4 f = *reinterpret_cast<const float4 *>(p);
                        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = cg + j < c_in ? p[j] : 0.f;
                    }
                }
                uint16_t h[4], l[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    h[j] = f32_to_bf16(v[j]);
                    l[j] = SPLIT ? f32_to_bf16(v[j] - bf16_to_f32(h[j])) : (uint16_t)0;
                }
                *reinterpret_cast<uint2 *>(&a_hi[row * PITCH + c4]) = make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
                if (SPLIT)
                    *reinterpret_cast<uint2 *>(&a_lo[row * PITCH + c4]) = make_uint2((uint32_t)l[0] | ((uint32_t)l[1] << 16), (uint32_t)l[2] | ((uint32_t)l[3] << 16));
            }
            __syncthreads();
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                // a 16-row tile none of whose rows has the offset is skipped (its LDS rows are zeros)
                const bool mine = s_nb[row0 + mt * 16 + l15] >= 0;
                if (__ballot(mine) == 0ull) continue;
                const int arow = (row0 + mt * 16 + l15) * PITCH + 8 * lq;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(&a_hi[arow + ks * 32]);
                    bf16x8 al = ah;
                    if (SPLIT) al = *reinterpret_cast<const bf16x8 *>(&a_lo[arow + ks * 32]);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[ks][nt], acc[mt][nt], 0, 0, 0);
                        if (SPLIT) {
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl[ks][nt], acc[mt][nt], 0, 0, 0);
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh[ks][nt], acc[mt][nt], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }
    // epilogue: accumulator element j of lane l is (row 4 (l >> 4) + j, column l & 15) of a 16 x 16 tile
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = col0 + nt * 16 + l15;
        const float b = bias ? bias[col] : 0.f;
        const float sc = scale ? scale[col] : 1.f, sh = scale ? shift[col] : 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t row = tile0 + row0 + mt * 16 + lq * 4 + j;
                if (row < n_out) {
                    float v = acc[mt][nt][j];
                    if (bias) v += b;
                    if (scale) v = v * sc + sh;
                    if (residual) v += residual[row * COUT + col];
                    if (relu) v = v > 0.f ? v : 0.f;
                    out[row * COUT + col] = v;
                }
            }
        }
    }
}

int cin_pad_of(int c_in) { return c_in <= 32 ? 32 : c_in; }
bool cin_ok(int c) { return c == 4 || c == 5 || c == 16 || c == 32 || c == 64 || c == 128; }
bool cout_ok(int c) { return c == 16 || c == 32 || c == 64 || c == 128; }
// the family: the narrow pairs above, plus the wide layers (128 -> 256) and (256 -> 256); C_in = 256 goes with C_out = 256 only
bool pair_ok(int c_in, int c_out) { return c_out == 256 ? (c_in == 128 || c_in == 256) : (cin_ok(c_in) && cout_ok(c_out)); }

struct RulesWs {
    float4 *pts;
    int32_t *unq_inv, *unq_key, *unq_cnt, *cells, *rowof, *counts;
    void *dyn;
    size_t dyn_bytes;
};
template <typename A> void rules_layout(A &a, RulesWs &w, int64_t ncand, size_t dyn_bytes) {
    w.pts = a.template take<float4>(ncand + 1);
    w.unq_inv = a.template take<int32_t>(ncand + 1);
    w.unq_key = a.template take<int32_t>(ncand + 1);
    w.unq_cnt = a.template take<int32_t>(ncand + 1);
    w.cells = a.template take<int32_t>(4 * (ncand + 1));
    w.rowof = a.template take<int32_t>(ncand + 1);
    w.counts = a.template take<int32_t>(4);
    w.dyn = a.template take<char>(dyn_bytes);
    w.dyn_bytes = dyn_bytes;
}

// LVQ_OK and a filled geometry, or the error code of the argument check
int rules_geom(int ndim, const int32_t *shape, int batch, const int32_t *kernel, const int32_t *stride, const int32_t *padding, int subm, RuleGeom &g) {
    if ((ndim != 2 && ndim != 3) || !shape || !kernel || batch <= 0) return LVQ_EINVAL;
    if (!subm && (!stride || !padding)) return LVQ_EINVAL;
    g.ndim = ndim; g.batch = batch; g.subm = subm ? 1 : 0;
    for (int a = 0; a < 3; ++a) { g.in[a] = g.out[a] = g.k[a] = g.s[a] = g.kc[a] = 1; g.p[a] = 0; }
    for (int j = 0; j < ndim; ++j) {
        const int a = 3 - ndim + j;
        g.in[a] = shape[j]; g.k[a] = kernel[j];
        if (g.in[a] <= 0 || g.k[a] <= 0 || g.k[a] > 3) return g.in[a] <= 0 || g.k[a] <= 0 ? LVQ_EINVAL : LVQ_EUNSUPPORTED;
        if (subm) {
            if (!(g.k[a] & 1)) return LVQ_EUNSUPPORTED;
            g.p[a] = g.k[a] / 2; g.out[a] = g.in[a];
        } else {
            g.s[a] = stride[j]; g.p[a] = padding[j];
            if (g.s[a] <= 0 || g.p[a] < 0) return LVQ_EINVAL;         // (p >= k is legal: conv_out with last_pad = 1 pads its 1-wide axes)
            const int num = g.in[a] + 2 * g.p[a] - g.k[a];
            if (num < 0) return LVQ_EINVAL;
            g.out[a] = num / g.s[a] + 1;
            g.kc[a] = (g.k[a] + g.s[a] - 1) / g.s[a];
        }
        if (g.in[a] >= (1 << 24) || g.out[a] >= (1 << 24)) return LVQ_EUNSUPPORTED;          // cells pass through fp32 exactly
    }
    if (batch >= (1 << 24)) return LVQ_EUNSUPPORTED;
    g.kvol = g.k[0] * g.k[1] * g.k[2];
    g.kcand = subm ? 1 : g.kc[0] * g.kc[1] * g.kc[2];
    // keys ((b D + z) H + y) W + x of the input AND of the output grid stay below 2^31
    const int64_t ks_in = (int64_t)batch * g.in[0] * g.in[1] * g.in[2], ks_out = (int64_t)batch * g.out[0] * g.out[1] * g.out[2];
    if (ks_in >= (1ll << 31) || ks_out >= (1ll << 31)) return LVQ_EOVERFLOW;
    return LVQ_OK;
}
size_t rules_dyn_bytes(const RuleGeom &g, int64_t ncand) {
    const int32_t grid3[3] = {g.out[0], g.out[1], g.out[2]}, grid2[3] = {g.out[1], g.out[2], 1};
    return lvq_voxelize_dynamic_workspace_bytes(ncand, g.batch, g.ndim == 3 ? grid3 : grid2, g.ndim);
}

}  // namespace

extern "C" size_t lvq_sparse_conv_rules_workspace_bytes(int64_t n_in, int ndim, const int32_t *spatial_shape_host, int batch, const int32_t *kernel_host,
                                                        const int32_t *stride_host, const int32_t *padding_host, int subm) {
    RuleGeom g;
    if (n_in < 0 || rules_geom(ndim, spatial_shape_host, batch, kernel_host, stride_host, padding_host, subm, g) != LVQ_OK) return 0;
    const int64_t ncand = n_in * g.kcand;
    if (ncand >= (1ll << 30)) return 0;
    const size_t dyn = rules_dyn_bytes(g, ncand);
    if (dyn == 0) return 0;
    SizerAdapter a;
    RulesWs w;
    rules_layout(a, w, ncand, dyn);
    return a.s.total();
}

extern "C" int lvq_sparse_conv_rules(const int32_t *indices, int64_t n_in, int ndim, const int32_t *spatial_shape_host, int batch,
                                     const int32_t *kernel_host, const int32_t *stride_host, const int32_t *padding_host, int subm, int64_t out_cap,
                                     int32_t *out_indices, int32_t *nbr, int32_t *n_out_dev, void *ws, size_t ws_bytes, lvq_stream_t stream) {
    RuleGeom g;
    if (n_in < 0 || out_cap < 0 || !n_out_dev) return LVQ_EINVAL;
    const int rcg = rules_geom(ndim, spatial_shape_host, batch, kernel_host, stride_host, padding_host, subm, g);
    if (rcg != LVQ_OK) return rcg;                                   // LVQ_EOVERFLOW included: nothing has been launched
    hipStream_t st = lvq_s(stream);
    if (n_in == 0) {
        hipMemsetAsync(n_out_dev, 0, sizeof(int32_t), st);
        return lvq_launch_status();
    }
    if (!indices || !nbr || (!subm && !out_indices)) return LVQ_EINVAL;
    const int64_t ncand = n_in * g.kcand;
    if (ncand >= (1ll << 30) || n_in * g.kvol >= (1ll << 31)) return LVQ_EUNSUPPORTED;
    const int64_t ks_out = (int64_t)batch * g.out[0] * g.out[1] * g.out[2];
    if (subm && out_cap < n_in) return LVQ_EINVAL;
    const size_t dyn = rules_dyn_bytes(g, ncand);
    if (dyn == 0) return LVQ_EOVERFLOW;
    LvqArena arena(ws, ws_bytes);
    RulesWs w;
    rules_layout(arena, w, ncand, dyn);
    if (!arena.ok) return LVQ_EWORKSPACE;
    const int32_t grid3[3] = {g.out[0], g.out[1], g.out[2]}, grid2[3] = {g.out[1], g.out[2], 1};
    const int32_t *grid = g.ndim == 3 ? grid3 : grid2;
    const float range[6] = {0.f, 0.f, 0.f, (float)grid[0], (float)grid[1], (float)grid[2]};
    const float vsize[3] = {1.f, 1.f, 1.f};
    const unsigned nbc = (unsigned)lvq_cdiv(ncand, 256);
    if (subm)
        hipLaunchKernelGGL(k_subm_pts, dim3(nbc), dim3(256), 0, st, indices, n_in, g, w.pts);
    else
        hipLaunchKernelGGL(k_rules_cand, dim3(nbc), dim3(256), 0, st, indices, n_in, g, w.pts);
    const int rc = lvq_voxelize_dynamic(reinterpret_cast<const float *>(w.pts), ncand, 4, batch, range, vsize, grid, g.ndim, w.unq_inv, nullptr,
                                        w.unq_key, w.unq_cnt, w.cells, w.counts, w.dyn, w.dyn_bytes, stream);
    if (rc != LVQ_OK) return rc;
    if (subm) {
        hipLaunchKernelGGL(k_subm_rowof, dim3(nbc), dim3(256), 0, st, w.unq_inv, n_in, w.rowof, n_out_dev);
        hipLaunchKernelGGL(k_subm_nbr, dim3((unsigned)lvq_cdiv(n_in * g.kvol, 256)), dim3(256), 0, st, indices, n_in, g, w.unq_key, w.counts, w.rowof, nbr);
    } else {
        int64_t cap = ncand < ks_out ? ncand : ks_out;               // the most rows there can be
        if (cap > out_cap) cap = out_cap;                            // rows past out_cap are not written; *n_out_dev still counts them
        hipLaunchKernelGGL(k_rules_out, dim3((unsigned)lvq_cdiv(cap * g.kvol, 256)), dim3(256), 0, st, w.unq_key, w.counts, cap, g, out_indices, nbr,
                           n_out_dev);
        hipLaunchKernelGGL(k_rules_scatter, dim3(nbc), dim3(256), 0, st, indices, n_in, g, w.unq_inv, w.counts, cap, nbr);
    }
    return lvq_launch_status();
}

extern "C" size_t lvq_sparse_conv_packed_elems(int c_out, int k_vol, int c_in) {
    if (!pair_ok(c_in, c_out) || k_vol <= 0 || k_vol > MAXK) return 0;
    return (size_t)k_vol * c_out * cin_pad_of(c_in);
}

extern "C" int lvq_sparse_conv_pack_weights(const float *weight, int c_out, int k_vol, int c_in, lvq_bf16 *w_hi, lvq_bf16 *w_lo, lvq_stream_t stream) {
    if (!weight || !w_hi || c_out <= 0 || c_in <= 0 || k_vol <= 0) return LVQ_EINVAL;
    const int64_t n = (int64_t)lvq_sparse_conv_packed_elems(c_out, k_vol, c_in);
    if (n == 0) return LVQ_EUNSUPPORTED;
    hipLaunchKernelGGL(k_pack_w, dim3((unsigned)lvq_cdiv(n, 256)), dim3(256), 0, lvq_s(stream), weight, c_out, k_vol, c_in, cin_pad_of(c_in), w_hi, w_lo);
    return lvq_launch_status();
}

namespace {
template <int CIN_PAD, bool SPLIT, typename... Args> int launch_cout(int c_out, unsigned nb, hipStream_t st, Args... args) {
    switch (c_out) {
    case 16: hipLaunchKernelGGL((k_sparse_conv<CIN_PAD, 16, SPLIT>), dim3(nb), dim3(256), 0, st, args...); break;
    case 32: hipLaunchKernelGGL((k_sparse_conv<CIN_PAD, 32, SPLIT>), dim3(nb), dim3(256), 0, st, args...); break;
    case 64: hipLaunchKernelGGL((k_sparse_conv<CIN_PAD, 64, SPLIT>), dim3(nb), dim3(256), 0, st, args...); break;
    case 128: hipLaunchKernelGGL((k_sparse_conv<CIN_PAD, 128, SPLIT>), dim3(nb), dim3(256), 0, st, args...); break;
    default: return LVQ_EUNSUPPORTED;
    }
    return lvq_launch_status();
}
template <int CIN_PAD, bool SPLIT, typename... Args> int launch_wide(unsigned nb, hipStream_t st, Args... args) {
    hipLaunchKernelGGL((k_sparse_conv<CIN_PAD, 256, SPLIT>), dim3(nb), dim3(256), 0, st, args...);
    return lvq_launch_status();
}
template <bool SPLIT, typename... Args> int launch_cin(int cin_pad, int c_out, unsigned nb, hipStream_t st, Args... args) {
    if (c_out == 256) return cin_pad == 256 ? launch_wide<256, SPLIT>(nb, st, args...) : launch_wide<128, SPLIT>(nb, st, args...);
    switch (cin_pad) {
    case 32: return launch_cout<32, SPLIT>(c_out, nb, st, args...);
    case 64: return launch_cout<64, SPLIT>(c_out, nb, st, args...);
    case 128: return launch_cout<128, SPLIT>(c_out, nb, st, args...);
    default: return LVQ_EUNSUPPORTED;
    }
}
}  // namespace

extern "C" int lvq_sparse_conv(const float *feat, int64_t n_in, int c_in, const int32_t *nbr, int k_vol, int64_t n_out_cap, const int32_t *n_out_dev,
                               const lvq_bf16 *w_hi, const lvq_bf16 *w_lo, int c_out, const float *bias, const float *scale, const float *shift,
                               const float *residual, int relu, float *out, lvq_stream_t stream) {
    if (n_in < 0 || n_out_cap < 0 || c_in <= 0 || c_out <= 0 || k_vol <= 0 || (scale == nullptr) != (shift == nullptr)) return LVQ_EINVAL;
    if (!pair_ok(c_in, c_out) || k_vol > MAXK) return LVQ_EUNSUPPORTED;
    if (n_out_cap == 0) return LVQ_OK;
    if (!nbr || !w_hi || !out || (n_in > 0 && !feat)) return LVQ_EINVAL;
    if (n_in >= (1ll << 31) || lvq_cdiv(n_out_cap, TILE_M) >= (1ll << 31)) return LVQ_EUNSUPPORTED;
    if ((((uintptr_t)w_hi | (uintptr_t)w_lo) & 15) || ((c_in & 3) == 0 && (((uintptr_t)feat) & 15))) return LVQ_EUNSUPPORTED;
    const unsigned nb = (unsigned)lvq_cdiv(n_out_cap, TILE_M);
    hipStream_t st = lvq_s(stream);
    if (w_lo)
        return launch_cin<true>(cin_pad_of(c_in), c_out, nb, st, feat, n_in, c_in, nbr, k_vol, n_out_cap, n_out_dev, w_hi, w_lo, bias, scale, shift, residual,
                                relu, out);
    return launch_cin<false>(cin_pad_of(c_in), c_out, nb, st, feat, n_in, c_in, nbr, k_vol, n_out_cap, n_out_dev, w_hi, w_lo, bias, scale, shift, residual,
                             relu, out);
}
