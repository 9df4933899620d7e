// csrc/bev_tiles.hip -- the sparse BEV key stream of VATLiDAR (vat_lidar.py:212-248 + vat_blocks.py:42), gfx950.
//
// A BEV cell whose 3x3 neighbourhood holds no pillar yields a token that depends on the weights only:
//     x[cell] = LayerNorm(proj(GELU(b_dw))) + PE[cell]        (refine conv -> 1x1 conv -> LayerNorm -> positional table)
// and so do its K|V rows.  At nuScenes densities that is ~3/4 of the 512 x 512 cells.  The stream is therefore cut into
// 8 x 8-cell TILES (64 keys = one attention K/V tile; key order is free under softmax, so keys run tile-major) of eight
// 2 x 4-cell PIECES (8 keys = 8 rows = one 1-KiB LDS-DMA piece of the attention kernel's K or V tile):
//   * a piece whose 4 x 6 halo holds no pillar is CLEAN: its K|V rows come from a per-model table that is computed once per
//     weights version by the very same kernels on an empty scene (bit-identical rows by construction);
//   * every other piece is LIVE: its tokens are computed here, its K|V rows by the GEMM over the compacted live rows, and the
//     attention kernel reads each piece of a tile through its own row offset (lvq_attention_bf16_tiled).
//   Live fraction of the bench scenes by granularity: 8 x 8 tiles 56.4 %, 4 x 4 43.5 %, 2 x 4 pieces 38.8 %, single cells 27.6 %.
// This file holds (1) the bookkeeping: live flags, compaction in (tile, scene, piece) order so that the scenes sharing a
// positional table tile run back to back, the per-(scene, tile, piece) source offsets; and (2) the fused token kernel: pillar gather + depthwise
// 3x3 + GELU (same tap order and fmaf chain as k_dwconv3x3_gelu) -> 1x1 conv on MFMA with W held in REGISTERS (column-
// stationary: wave w owns N/8 output columns, so W is never re-read and needs no LDS) -> LayerNorm (per-wave (mean, M2)
// partials merged with Chan's formula) -> + positional table -> bf16 rows, without any intermediate in HBM.
#include "common.h"
#include <type_traits>
#include <utility>

namespace bt {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
    bf16x2_t p = {(__bf16)a, (__bf16)b};
    return *reinterpret_cast<uint32_t *>(&p);
}
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_f16(float a, float b) {          // round to nearest even (not v_cvt_pkrtz)
    f16x2_t p = {(_Float16)a, (_Float16)b};
    return __builtin_bit_cast(uint32_t, p);
}

constexpr int TS = 8, TCELLS = 64;                 // tile side (cells), keys per tile
constexpr int NPIECE = 8, PCELLS = 8;              // pieces per tile, cells per piece (2 rows x 4 columns)
constexpr int PH = 4, PW = 6, PHALO = PH * PW;     // a piece's halo (2 + 2 rows, 4 + 2 columns)
constexpr int NSLOT = NPIECE * PHALO;              // halo slots of one 8-piece work item (192)
constexpr int CNT_BLOCK = 1024;                    // pieces per counting block

// origin (y, x) of piece p of tile t: row pair p >> 1, column half p & 1
__device__ __forceinline__ void piece_origin(int t, int p, int tw, int &y0, int &x0) {
    y0 = (t / tw) * TS + (p >> 1) * 2;
    x0 = (t % tw) * TS + (p & 1) * 4;
}

// dirty mask of the piece with flat index i = (t * S + s) * 8 + p: bit j = 4 cy + cx is set when cell (cy, cx) of the 2 x 4 piece has a
// pillar in its 3 x 3 neighbourhood (its token depends on the scene); 0 = the whole piece is clean; `force`: all 8 bits
__device__ __forceinline__ unsigned piece_mask(const int32_t *__restrict__ idx, int64_t i, int S, int H, int W, int force) {
    if (force) return 0xffu;
    const int tw = W / TS;
    const int p = (int)(i & 7);
    const int64_t ts = i >> 3;
    const int t = (int)(ts / S), s = (int)(ts - (int64_t)t * S);
    int y0, x0;
    piece_origin(t, p, tw, y0, x0);
    const int32_t *plane = idx + (int64_t)s * H * W;
    unsigned occ[PH];                                            // occupancy bits of the 4 x 6 halo, one word per row
#pragma unroll
    for (int r = 0; r < PH; ++r) {
        occ[r] = 0;
        const int gy = y0 - 1 + r;
        if (gy < 0 || gy >= H) continue;
        // columns x0 .. x0 + 3 are one aligned 16-byte word (x0 and W are multiples of 4), the two flanks single words
        const int32_t *row = plane + (int64_t)gy * W + x0;
        const int4 mid = *reinterpret_cast<const int4 *>(row);
        occ[r] = (mid.x >= 0 ? 2u : 0u) | (mid.y >= 0 ? 4u : 0u) | (mid.z >= 0 ? 8u : 0u) | (mid.w >= 0 ? 16u : 0u);
        if (x0 > 0 && row[-1] >= 0) occ[r] |= 1u;
        if (x0 + 4 < W && row[4] >= 0) occ[r] |= 32u;
    }
    unsigned m = 0;
#pragma unroll
    for (int cy = 0; cy < 2; ++cy) {
        const unsigned rows = occ[cy] | occ[cy + 1] | occ[cy + 2];
#pragma unroll
        for (int cx = 0; cx < 4; ++cx)
            if (rows & (7u << cx)) m |= 1u << (4 * cy + cx);
    }
    return m;
}

// ---- pass 1: live pieces and dirty rows per block of CNT_BLOCK flat indices: block_cnt[2 b] / [2 b + 1] ----
__global__ void __launch_bounds__(256) k_piece_count(const int32_t *__restrict__ idx, int S, int H, int W, int force, int64_t total,
                                                     int32_t *__restrict__ block_cnt, uint8_t *__restrict__ masks) {
    __shared__ int wsum[4][2];
    int c = 0, dcount = 0;
#pragma unroll
    for (int u = 0; u < CNT_BLOCK / 256; ++u) {
        const int64_t i = (int64_t)blockIdx.x * CNT_BLOCK + u * 256 + threadIdx.x;
        if (i < total) {
            const unsigned m = piece_mask(idx, i, S, H, W, force);
            masks[i] = (uint8_t)m;                                // pass 2 reads the byte instead of the 24 halo words again
            c += m ? 1 : 0;
            dcount += __popc(m);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { c += __shfl_xor(c, o); dcount += __shfl_xor(dcount, o); }
    if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6][0] = c; wsum[threadIdx.x >> 6][1] = dcount; }
    __syncthreads();
    if (threadIdx.x == 0) {
        block_cnt[2 * blockIdx.x] = wsum[0][0] + wsum[1][0] + wsum[2][0] + wsum[3][0];
        block_cnt[2 * blockIdx.x + 1] = wsum[0][1] + wsum[1][1] + wsum[2][1] + wsum[3][1];
    }
}

// ---- pass 2: every block re-sums the block counts in front of it (<= a few thousand L2-resident values), recomputes its masks and
// writes, in (tile, scene, piece) order,
//   live_list[k]      = flat index (t * S + s) * 8 + p of the k-th live piece
//   piece_dirty[k]    = (first dirty-row number of the piece, its dirty mask): the piece's dirty cells own consecutive rows of the
//                       compact row buffer in cell order
//   row_src[s * HW + 64 t + 8 p + j] = row_base + (dirty-row number) for a dirty cell, 64 t + 8 p + j (its row in the table) otherwise
//   counts[0] = live pieces, counts[1] = rows of the live pieces (8 x), counts[2] = dirty rows, by the last block
__global__ void __launch_bounds__(256) k_piece_compact(const int32_t *__restrict__ idx, int S, int H, int W, int force, int64_t total,
                                                       const int32_t *__restrict__ block_cnt, const uint8_t *__restrict__ masks, int nblocks, int row_base,
                                                       int32_t *__restrict__ live_list, int2 *__restrict__ piece_dirty, int32_t *__restrict__ row_src,
                                                       int32_t *__restrict__ counts) {
    __shared__ int wsum[4][2];
    __shared__ int l_base[2];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int c = 0, dcount = 0;
    for (int b = tid; b < (int)blockIdx.x; b += 256) { c += block_cnt[2 * b]; dcount += block_cnt[2 * b + 1]; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { c += __shfl_xor(c, o); dcount += __shfl_xor(dcount, o); }
    if (lane == 0) { wsum[wid][0] = c; wsum[wid][1] = dcount; }
    __syncthreads();
    if (tid == 0) {
        l_base[0] = wsum[0][0] + wsum[1][0] + wsum[2][0] + wsum[3][0];
        l_base[1] = wsum[0][1] + wsum[1][1] + wsum[2][1] + wsum[3][1];
    }
    __syncthreads();
    int base = l_base[0], dbase = l_base[1];
    const int nt = (H / TS) * (W / TS);
    const int64_t hw = (int64_t)H * W;
    for (int u = 0; u < CNT_BLOCK / 256; ++u) {
        const int64_t i = (int64_t)blockIdx.x * CNT_BLOCK + u * 256 + tid;
        const unsigned msk = i < total ? (unsigned)masks[i] : 0u;
        const bool live = msk != 0;
        const unsigned long long bal = __ballot(live);
        const int nd = __popc(msk);
        int inc = nd;                                             // inclusive wave scan of the dirty-row counts
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int n = __shfl_up(inc, o); if (lane >= o) inc += n; }
        __syncthreads();
        if (lane == 63) { wsum[wid][0] = __popcll(bal); wsum[wid][1] = inc; }
        __syncthreads();
        int wb = 0, tot = 0, dwb = 0, dtot = 0;
        for (int q = 0; q < 4; ++q) { if (q < wid) { wb += wsum[q][0]; dwb += wsum[q][1]; } tot += wsum[q][0]; dtot += wsum[q][1]; }
        if (i < total) {
            const int p = (int)(i & 7);
            const int64_t ts = i >> 3;
            const int t = (int)(ts / S), sc = (int)(ts - (int64_t)t * S);
            const int e0 = t * TCELLS + p * PCELLS;               // the piece's first row in the table (tile-major key order)
            const int d0 = dbase + dwb + inc - nd;               // its first dirty-row number
            if (live) {
                const int k = base + wb + __popcll(bal & ((1ull << lane) - 1ull));
                live_list[k] = (int32_t)i;
                piece_dirty[k] = make_int2(d0, (int)msk);
            }
            int32_t rs[PCELLS];
#pragma unroll
            for (int j = 0; j < PCELLS; ++j)
                rs[j] = (msk >> j) & 1u ? row_base + d0 + __popc(msk & ((1u << j) - 1u)) : e0 + j;
            int4 *dst = reinterpret_cast<int4 *>(row_src + (int64_t)sc * hw + e0);
            dst[0] = make_int4(rs[0], rs[1], rs[2], rs[3]);
            dst[1] = make_int4(rs[4], rs[5], rs[6], rs[7]);
        }
        base += tot;
        dbase += dtot;
    }
    if ((int)blockIdx.x == nblocks - 1 && tid == 0) { counts[0] = base; counts[1] = base * PCELLS; counts[2] = dbase; }
}

// ---- pass 3 (optional): the per-scene PAIR list of lvq_attention_bf16_tiled_signed.  One workgroup per scene compacts the dirty rows of
// row_src in stream order; pair tile j of scene s holds dirty rows 32 j .. 32 j + 31 twice:
//   pair_src[(s * cap + j) * 64 + u]      = the computed row (>= row_base)                     (u = 0..31: keys 0..31 of the tile, added)
//   pair_src[(s * cap + j) * 64 + 32 + u] = the table row of the same cell (its position e)    (keys 32..63: subtracted)
// The last tile is padded with table row 0 in BOTH halves (+c - c).  pair_info[2 s] = pair tiles (or 0), pair_info[2 s + 1] = 1
// when the signed stream is shorter than the scene's full stream of nt tiles (and fits cap), else 0 = use the full stream.
constexpr int PAIR_NT = 1024;
__global__ void __launch_bounds__(PAIR_NT) k_scene_pairs(const int32_t *__restrict__ row_src, int nt, int row_base, int cap, int32_t *__restrict__ pair_src,
                                                         int32_t *__restrict__ pair_info) {
    __shared__ int wsum[PAIR_NT / 64];
    __shared__ int l_run;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ne = nt * TCELLS;                                  // rows of this scene
    const int32_t *src = row_src + (int64_t)s * ne;
    int32_t *dst = pair_src + (int64_t)s * cap * TCELLS;
    const int cap_r = cap * 32;                                  // dirty rows the list can hold
    if (tid == 0) l_run = 0;
    __syncthreads();
    for (int e0 = 0; e0 < ne; e0 += PAIR_NT * 4) {
        const int e = e0 + tid * 4;
        int4 v = make_int4(0, 0, 0, 0);
        if (e < ne) v = *reinterpret_cast<const int4 *>(src + e);
        const int32_t vv[4] = {v.x, v.y, v.z, v.w};
        int c = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) c += (e < ne && vv[u] >= row_base) ? 1 : 0;
        int inc = c;                                             // inclusive wave scan
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int n = __shfl_up(inc, o); if (lane >= o) inc += n; }
        if (lane == 63) wsum[wid] = inc;
        __syncthreads();
        int wb = 0, tot = 0;
#pragma unroll
        for (int q = 0; q < PAIR_NT / 64; ++q) { if (q < wid) wb += wsum[q]; tot += wsum[q]; }
        int j = l_run + wb + inc - c;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (e < ne && vv[u] >= row_base) {
                if (j < cap_r) {
                    dst[(j >> 5) * TCELLS + (j & 31)] = vv[u];
                    dst[(j >> 5) * TCELLS + 32 + (j & 31)] = e + u;
                }
                ++j;
            }
        __syncthreads();
        if (tid == 0) l_run += tot;
        __syncthreads();
    }
    const int n_dirty = l_run, n_pt = (n_dirty + 31) >> 5;
    const bool use = n_pt < nt && n_pt <= cap;
    if (use && tid < 32 && n_dirty + tid < n_pt * 32) {           // padding of the last pair tile
        const int j = n_dirty + tid;
        dst[(j >> 5) * TCELLS + (j & 31)] = 0;
        dst[(j >> 5) * TCELLS + 32 + (j & 31)] = 0;
    }
    if (tid == 0) { pair_info[2 * s] = use ? n_pt : 0; pair_info[2 * s + 1] = use ? 1 : 0; }
}

// The same lists from many workgroups per scene (one workgroup per scene walks 262 144 words in 64 dependent rounds: 123 us of a 20 ms
// step at 32 scenes).  A scene is cut into <= 64 chunks of whole 1024-word rounds; pass 1 counts the dirty rows per chunk, pass 2 gives
// every chunk its starting position (the sum of the counts before it) and compacts it.  The chunk counts live in the LAST tile slot of
// the scene's list (cap >= nt: a list that is used has fewer than nt tiles, so that slot is never part of one); entries are written
// for positions below (cap - 1) * 32 only.
constexpr int PAIR2_NT = 256;
__global__ void __launch_bounds__(PAIR2_NT) k_scene_pair_count(const int32_t *__restrict__ row_src, int nt, int row_base, int cap, int chunk,
                                                               int32_t *__restrict__ pair_src) {
    __shared__ int wsum[PAIR2_NT / 64];
    const int ch = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ne = nt * TCELLS;
    const int32_t *src = row_src + (int64_t)s * ne;
    const int e_end = (ch + 1) * chunk < ne ? (ch + 1) * chunk : ne;
    int c = 0;
    for (int e = ch * chunk + tid * 4; e < e_end; e += PAIR2_NT * 4) {
        const int4 v = *reinterpret_cast<const int4 *>(src + e);
        c += (v.x >= row_base) + (v.y >= row_base) + (v.z >= row_base) + (v.w >= row_base);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) wsum[wid] = c;
    __syncthreads();
    if (tid == 0) pair_src[((int64_t)s * cap + (cap - 1)) * TCELLS + ch] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
__global__ void __launch_bounds__(PAIR2_NT) k_scene_pair_write(const int32_t *__restrict__ row_src, int nt, int row_base, int cap, int chunk, int nch,
                                                               int32_t *__restrict__ pair_src, int32_t *__restrict__ pair_info) {
    __shared__ int wsum[PAIR2_NT / 64];
    __shared__ int l_start[2];
    const int ch = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ne = nt * TCELLS;
    const int32_t *src = row_src + (int64_t)s * ne;
    int32_t *dst = pair_src + (int64_t)s * cap * TCELLS;
    if (tid < 64) {                                              // start = dirty rows of the chunks before this one, total = of all
        const int v = tid < nch ? dst[(int64_t)(cap - 1) * TCELLS + tid] : 0;
        int before = tid < ch ? v : 0, all = v;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { before += __shfl_xor(before, o); all += __shfl_xor(all, o); }
        if (tid == 0) { l_start[0] = before; l_start[1] = all; }
    }
    __syncthreads();
    int run = l_start[0];
    const int n_dirty = l_start[1];
    const int lim = (cap - 1) * 32;
    const int e_end = (ch + 1) * chunk < ne ? (ch + 1) * chunk : ne;
    for (int e0 = ch * chunk; e0 < e_end; e0 += PAIR2_NT * 4) {
        const int e = e0 + tid * 4;
        int4 v = make_int4(0, 0, 0, 0);
        if (e < e_end) v = *reinterpret_cast<const int4 *>(src + e);
        const int32_t vv[4] = {v.x, v.y, v.z, v.w};
        int c = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) c += (e < e_end && vv[u] >= row_base) ? 1 : 0;
        int inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int n = __shfl_up(inc, o); if (lane >= o) inc += n; }
        __syncthreads();                                         // (wsum of the previous round has been read)
        if (lane == 63) wsum[wid] = inc;
        __syncthreads();
        int wb = 0, tot = 0;
#pragma unroll
        for (int q = 0; q < PAIR2_NT / 64; ++q) { if (q < wid) wb += wsum[q]; tot += wsum[q]; }
        int j = run + wb + inc - c;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (e < e_end && vv[u] >= row_base) {
                if (j < lim) {
                    dst[(j >> 5) * TCELLS + (j & 31)] = vv[u];
                    dst[(j >> 5) * TCELLS + 32 + (j & 31)] = e + u;
                }
                ++j;
            }
        run += tot;
    }
    if (ch == 0) {
        const int n_pt = (n_dirty + 31) >> 5;
        const bool use = n_pt < nt && n_pt <= cap - 1;
        if (use && tid < 32 && n_dirty + tid < n_pt * 32) {       // padding of the last pair tile
            const int j = n_dirty + tid;
            dst[(j >> 5) * TCELLS + (j & 31)] = 0;
            dst[(j >> 5) * TCELLS + 32 + (j & 31)] = 0;
        }
        if (tid == 0) { pair_info[2 * s] = use ? n_pt : 0; pair_info[2 * s + 1] = use ? 1 : 0; }
    }
}

// ---- shared subtraction (lvq_bev_shared_lists, DESIGN 3.2 "Shared subtraction"): a cell that is dirty in m of the S scenes of a batch
// with 2 m > S + 1 goes into the shared set G.  Its table row is subtracted ONCE for the whole batch (the G list, streamed with B = 1) and
// added back in the scenes where the cell is clean.  A scene's list: pair tiles (32 computed rows | the 32 table rows of the same cells) of its
// dirty cells outside G, then ONE plus slot per cell of G in key order (the computed row where the scene is dirty, the table row where it is
// clean) in tiles of 64, then at most two remainder tiles of 32 plus slots whose second half is ignored.  Every scene has exactly |G| plus
// slots and the G list has |G| rows, so all of them pad to the same multiple of 32 with table row 0: the G list subtracts those copies
// of row 0 and every scene that uses its list adds them back.
constexpr int SH_NT = 256;
// pass 1: flag[e] = 1 when cell e is in G
__global__ void __launch_bounds__(SH_NT) k_shared_flags(const int32_t *__restrict__ row_src, int S, int ne, int row_base, uint8_t *__restrict__ flag) {
    const int e = ((int)blockIdx.x * SH_NT + (int)threadIdx.x) * 4;
    if (e >= ne) return;
    int m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    for (int s = 0; s < S; ++s) {
        const int4 v = *reinterpret_cast<const int4 *>(row_src + (int64_t)s * ne + e);
        m0 += v.x >= row_base; m1 += v.y >= row_base; m2 += v.z >= row_base; m3 += v.w >= row_base;
    }
    const int thr = S + 1;
    *reinterpret_cast<uint32_t *>(flag + e) = (uint32_t)(2 * m0 > thr) | ((uint32_t)(2 * m1 > thr) << 8) | ((uint32_t)(2 * m2 > thr) << 16) |
                                              ((uint32_t)(2 * m3 > thr) << 24);
}
// pass 2: per scene and chunk the dirty cells outside G (cnt[s * 64 + ch]) and inside G (cnt[(S + 1 + s) * 64 + ch]); per chunk the cells of
// G (cnt[S * 64 + ch], by the blocks of scene 0)
__global__ void __launch_bounds__(SH_NT) k_shared_count(const int32_t *__restrict__ row_src, const uint8_t *__restrict__ flag, int S, int nt, int row_base,
                                                        int chunk, int32_t *__restrict__ cnt) {
    __shared__ int wsum[SH_NT / 64][3];
    const int ch = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ne = nt * TCELLS;
    const int32_t *src = row_src + (int64_t)s * ne;
    const int e_end = (ch + 1) * chunk < ne ? (ch + 1) * chunk : ne;
    int c = 0, g = 0, dg = 0;
    for (int e = ch * chunk + tid * 4; e < e_end; e += SH_NT * 4) {
        const int4 v = *reinterpret_cast<const int4 *>(src + e);
        const uint32_t f = *reinterpret_cast<const uint32_t *>(flag + e);
        const int f0 = f & 1, f1 = (f >> 8) & 1, f2 = (f >> 16) & 1, f3 = (f >> 24) & 1;
        c += (v.x >= row_base && !f0) + (v.y >= row_base && !f1) + (v.z >= row_base && !f2) + (v.w >= row_base && !f3);
        dg += (v.x >= row_base && f0) + (v.y >= row_base && f1) + (v.z >= row_base && f2) + (v.w >= row_base && f3);
        g += f0 + f1 + f2 + f3;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { c += __shfl_xor(c, o); g += __shfl_xor(g, o); dg += __shfl_xor(dg, o); }
    if (lane == 0) { wsum[wid][0] = c; wsum[wid][1] = g; wsum[wid][2] = dg; }
    __syncthreads();
    if (tid == 0) {
        cnt[s * 64 + ch] = wsum[0][0] + wsum[1][0] + wsum[2][0] + wsum[3][0];
        cnt[(S + 1 + s) * 64 + ch] = wsum[0][2] + wsum[1][2] + wsum[2][2] + wsum[3][2];
        if (s == 0) cnt[S * 64 + ch] = wsum[0][1] + wsum[1][1] + wsum[2][1] + wsum[3][1];
    }
}
// pass 3: the lists.  First the batch's cost rule, from the counts alone (every workgroup takes the same decision): with a(s) / b(s) the tiles
// scene s would stream with its plain pair list / with the shared lists (n_tiles when the list is not shorter than the full stream), G is
// used only when sum_s (a(s) - b(s)) exceeds the tiles of the G list itself -- a batch of mostly dirty scenes has a large G that hardly
// shortens any list.  Otherwise G counts as empty: plain pair lists, an empty G list.  blockIdx.y = S writes the G list (no pair tiles, the table row of every cell of G).  info[4 s] = tiles (0 when unused),
// [4 s + 1] = use, [4 s + 2] = first tile whose second half is ADDED (= pair tiles), [4 s + 3] = first tile whose second half is IGNORED.
__global__ void __launch_bounds__(SH_NT) k_shared_write(const int32_t *__restrict__ row_src, const uint8_t *__restrict__ flag, int S, int nt, int row_base,
                                                        int cap, int chunk, int nch, const int32_t *__restrict__ cnt, int32_t *__restrict__ list_src,
                                                        int32_t *__restrict__ info) {
    __shared__ int wsum[SH_NT / 64];
    __shared__ int l_start[6];
    __shared__ int l_gain;
    const int ch = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const bool isg = s == S;
    const int ne = nt * TCELLS;
    const int32_t *src = row_src + (int64_t)(isg ? 0 : s) * ne;
    int32_t *dst = list_src + (int64_t)s * cap * TCELLS;
    if (tid < 64) {
        const int vp = (tid < nch && !isg) ? cnt[s * 64 + tid] : 0, vg = tid < nch ? cnt[S * 64 + tid] : 0;
        const int vd = (tid < nch && !isg) ? cnt[(S + 1 + s) * 64 + tid] : 0;
        int bp = tid < ch ? vp : 0, ap = vp, bg = tid < ch ? vg : 0, ag = vg, bd = tid < ch ? vd : 0, ad = vd;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            bp += __shfl_xor(bp, o); ap += __shfl_xor(ap, o); bg += __shfl_xor(bg, o); ag += __shfl_xor(ag, o);
            bd += __shfl_xor(bd, o); ad += __shfl_xor(ad, o);
        }
        if (tid == 0) { l_start[0] = bp; l_start[1] = ap; l_start[2] = bg; l_start[3] = ag; l_start[4] = bd; l_start[5] = ad; l_gain = 0; }
    }
    __syncthreads();
    const int g_tiles = (l_start[3] >> 6) + (((l_start[3] + 31) >> 5) - 2 * (l_start[3] >> 6));      // tiles of the G list
    for (int sc = tid; sc < S; sc += SH_NT) {
        int np = 0, nd = 0;
        for (int q = 0; q < nch; ++q) { np += cnt[sc * 64 + q]; nd += cnt[(S + 1 + sc) * 64 + q]; }
        int a = (np + nd + 31) >> 5, b = ((np + 31) >> 5) + g_tiles;
        a = a < nt ? a : nt;
        b = b < nt ? b : nt;
        if (a != b) atomicAdd(&l_gain, a - b);
    }
    __syncthreads();
    const bool share = l_gain > g_tiles;
    int run_p = l_start[0] + (share ? 0 : l_start[4]), run_g = share ? l_start[2] : 0;
    const int n_pair = l_start[1] + (share ? 0 : l_start[5]), n_g = share ? l_start[3] : 0;
    const int n_pt = (n_pair + 31) >> 5;                         // pair tiles
    const int n_full = n_g >> 6, n_half = (n_g + 31) >> 5;       // tiles of 64 plus slots; 32-slot halves in all
    const int n_all = n_pt + n_full + (n_half - 2 * n_full);
    // plus slot j (its cell's rank in G) -> word of the list, or -1 past the capacity
    auto plus_pos = [&](int j) {
        const int r = j - 64 * n_full;
        const int t = r < 0 ? n_pt + (j >> 6) : n_pt + n_full + (r >> 5);
        return t < cap ? t * TCELLS + (r < 0 ? (j & 63) : (r & 31)) : -1;
    };
    const int e_end = (ch + 1) * chunk < ne ? (ch + 1) * chunk : ne;
    for (int e0 = ch * chunk; e0 < e_end; e0 += SH_NT * 4) {
        const int e = e0 + tid * 4;
        int4 v = make_int4(-1, -1, -1, -1);
        uint32_t f = 0;
        if (e < e_end) {
            if (!isg) v = *reinterpret_cast<const int4 *>(src + e);
            if (share) f = *reinterpret_cast<const uint32_t *>(flag + e);
        }
        const int32_t vv[4] = {v.x, v.y, v.z, v.w};
        int c = 0;                                               // pair entries | plus entries << 16 of this thread
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool g = (f >> (8 * u)) & 1u, d = !isg && e < e_end && vv[u] >= row_base;
            c += (d && !g ? 1 : 0) + (g ? 0x10000 : 0);
        }
        int inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int n = __shfl_up(inc, o); if (lane >= o) inc += n; }
        __syncthreads();                                         // (wsum of the previous round has been read)
        if (lane == 63) wsum[wid] = inc;
        __syncthreads();
        int wb = 0, tot = 0;
#pragma unroll
        for (int q = 0; q < SH_NT / 64; ++q) { if (q < wid) wb += wsum[q]; tot += wsum[q]; }
        const int excl = wb + inc - c;
        int jp = run_p + (excl & 0xffff), jg = run_g + (excl >> 16);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool g = (f >> (8 * u)) & 1u, d = !isg && e < e_end && vv[u] >= row_base;
            if (g) {
                const int w = plus_pos(jg);
                if (w >= 0) dst[w] = d ? vv[u] : e + u;
                ++jg;
            } else if (d) {
                if ((jp >> 5) < cap) {
                    dst[(jp >> 5) * TCELLS + (jp & 31)] = vv[u];
                    dst[(jp >> 5) * TCELLS + 32 + (jp & 31)] = e + u;
                }
                ++jp;
            }
        }
        run_p += tot & 0xffff;
        run_g += tot >> 16;
    }
    if (ch == 0) {
        const bool use = n_all <= cap && (isg || n_all < nt);
        if (use && tid < 32) {
            if (n_pair + tid < n_pt * 32) {                       // padding of the last pair tile: +row 0 - row 0
                const int j = n_pair + tid;
                dst[(j >> 5) * TCELLS + (j & 31)] = 0;
                dst[(j >> 5) * TCELLS + 32 + (j & 31)] = 0;
            }
            if (n_g + tid < n_half * 32) dst[plus_pos(n_g + tid)] = 0;      // plus padding: the same number of copies of row 0 in every list
            for (int t = n_pt + n_full; t < n_all; ++t) dst[t * TCELLS + 32 + tid] = 0;   // the ignored halves (any row in bounds)
        }
        if (tid == 0) {
            info[4 * s] = use ? n_all : 0; info[4 * s + 1] = use ? 1 : 0;
            info[4 * s + 2] = n_pt; info[4 * s + 3] = n_pt + n_full;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// fused token kernel.  512 threads = 8 waves; persistent over the live list.  A work item ("group") = 8 consecutive live pieces =
// 64 rows = four 16-row MFMA groups; its pieces may belong to different tiles / scenes, each brings its own 4 x 6 halo.
//   J   = 16-column MFMA tiles per wave (N = 128 J: 768 -> 6, 1024 -> 8, 512 -> 4, 256 -> 2; even, so a lane's 8 J output bytes stay 16-byte aligned)
//   X3  = operands hi + lo (t and W), products hi*hi + hi*lo + lo*hi
//   OLO = also write the lo half of x (bf16x3 consumers); the mixed mode keeps x plain
// Product orientation: A = W rows (the wave's columns), B = t tile (16 cells x 64 k) -> C[row = column, col = cell]; with the
// W row permutation n = 16 J w + 4 J (m >> 2) + 4 j + (m & 3) for A row m of column tile j, lane (cell = l & 15, g4 = l >> 4)
// owns the 4 J CONSECUTIVE columns 16 J w + 4 J g4 .. of its cell: positional-table reads are J float4 and the output leaves
// as J/2 (or so) 16-byte stores, 4 lanes covering 32 J contiguous bytes of a row.
// Per group: [B1: conv tokens ready] DMA of the next group's pillar rows, pass 1 (MFMA -> per-wave (mean, M2)), [B2] conv of the
// next group (LDS only), pass 2 (MFMA again -> normalise -> + table -> store): two barriers, no HBM intermediate.
// ---------------------------------------------------------------------------------------------------------
struct TokArgs {
    const float *feat;            // [M, 64] pillar features
    const int32_t *idx;           // [S, H, W] pillar row or -1
    const int32_t *live_list;     // flat piece indices (t * S + s) * 8 + p
    const int32_t *counts;        // counts[0] = live pieces
    const float *w9, *b9;         // depthwise conv [64, 9], [64]
    const uint16_t *wh, *wl;      // 1x1 conv [N, 64] bf16 hi / lo
    const float *bias, *gamma, *beta, *pe;     // [N], [N], [N], positional table [H*W (tile-major), N]
    float eps;
    int S, H, W;
    const int2 *piece_dirty;      // per live piece: (first dirty-row number, dirty mask)
    uint16_t *xh, *xl;            // [dirty rows, N]: the dirty cells of live piece k own rows piece_dirty[k].x .. in cell order
};

template <int J, bool X3, bool OLO>
__global__ void __launch_bounds__(512) k_tile_tokens(TokArgs a) {
    constexpr int N = 128 * J, C = 64, NWV = 8;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    // LDS map
    uint16_t *t_hi = reinterpret_cast<uint16_t *>(smem);                      // [2][64][64] bf16, 128-byte rows, chunk-swizzled
    uint16_t *t_lo = t_hi + 2 * TCELLS * C;                                   // [2][64][64]
    float *halo = reinterpret_cast<float *>(t_lo + 2 * TCELLS * C);           // [192][64] fp32 pillar rows of the 8 halos (live slots only)
    int32_t *idxh = reinterpret_cast<int32_t *>(halo + NSLOT * C);            // [2][256]: 192 halo indices + 8 piece codes at [200..207]
    float *part = reinterpret_cast<float *>(idxh + 2 * 256);                  // [2][8 waves][64 cells][2]
    float *pbias = part + 2 * NWV * TCELLS * 2, *pgam = pbias + N, *pbet = pgam + N;
    float *w9s = pbet + N;                                                    // [9][64]
    float *b9s = w9s + 9 * C;                                                 // [64]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l15 = lane & 15, g4 = lane >> 4;
    const int tw = a.W / TS;
    const int n_live = a.counts[0];                             // live pieces
    const int64_t n_groups = ((int64_t)n_live + NPIECE - 1) / NPIECE;

    for (int e = tid; e < N; e += 512) { pbias[e] = a.bias ? a.bias[e] : 0.f; pgam[e] = a.gamma[e]; pbet[e] = a.beta ? a.beta[e] : 0.f; }
    for (int e = tid; e < 9 * C; e += 512) w9s[e] = a.w9[(e % C) * 9 + e / C];
    if (tid < C) b9s[tid] = a.b9 ? a.b9[tid] : 0.f;

    // W fragments (A operand) in registers: lane (m = l15, kc = g4) holds W[n(m, j)][8 kc .. +7] and [32 + 8 kc .. +7]
    bf16x8 wf[J][2], wfl[X3 ? J : 1][2];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int n = 16 * J * wid + 4 * J * (l15 >> 2) + 4 * j + (l15 & 3);
        wf[j][0] = *reinterpret_cast<const bf16x8 *>(a.wh + (int64_t)n * C + 8 * g4);
        wf[j][1] = *reinterpret_cast<const bf16x8 *>(a.wh + (int64_t)n * C + 32 + 8 * g4);
        if (X3) {
            wfl[j][0] = *reinterpret_cast<const bf16x8 *>(a.wl + (int64_t)n * C + 8 * g4);
            wfl[j][1] = *reinterpret_cast<const bf16x8 *>(a.wl + (int64_t)n * C + 32 + 8 * g4);
        }
    }
    const int col0 = 16 * J * wid + 4 * J * g4;                  // this lane's first column (4 J consecutive ones)

    // work order: the list is in (tile, scene, piece) order, so neighbouring groups need the same rows of the positional table.  Each
    // XCD (hardware deals block ids round-robin over the 8 XCDs, each with its own 4 MiB L2) takes one CONTIGUOUS eighth of the list
    // and its workgroups walk it INTERLEAVED (workgroup r of R takes groups r, r + R, ...): at any time the XCD works on ~R
    // consecutive groups = a few tiles, whose table rows (192 KB per tile) are then L2 hits for everyone but the first reader.  (One
    // contiguous run per workgroup keeps 32 different table tiles in flight per XCD -- 6 MB, more than the L2.)
    const int nxcd = gridDim.x >= 8 && gridDim.x % 8 == 0 ? 8 : 1;
    const int xcd = (int)blockIdx.x % nxcd, wg_r = (int)blockIdx.x / nxcd, wg_R = (int)gridDim.x / nxcd;
    const int64_t per_x = (n_groups + nxcd - 1) / nxcd;
    const int64_t x_begin = (int64_t)xcd * per_x, x_end = x_begin + per_x < n_groups ? x_begin + per_x : n_groups;
    const int64_t g_begin = x_begin + wg_r, g_end = x_end, g_step = wg_R;       // this workgroup: g_begin, g_begin + g_step, ... < g_end
    // halo index of slot tid (< 192) of group g: piece j = tid / 24 (code = live_list[8 g + j]), halo cell tid % 24; threads with
    // tid % 24 == 0 also return the piece code (-1 past the end of the list)
    auto load_idx = [&](int64_t g, int &code_out) -> int {
        code_out = -1;
        if (tid >= NSLOT) return -1;
        const int j = tid / PHALO, hc = tid - j * PHALO;
        const int64_t k = g * NPIECE + j;
        if (k >= n_live) return -1;
        const int code = a.live_list[k];
        code_out = code;
        const int p = code & 7, ts = code >> 3, t = ts / a.S, sc = ts - t * a.S;
        int y0, x0;
        piece_origin(t, p, tw, y0, x0);
        const int gy = y0 - 1 + hc / PW, gx = x0 - 1 + hc % PW;
        return (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) ? a.idx[((int64_t)sc * a.H + gy) * a.W + gx] : -1;
    };
    auto store_idx = [&](int32_t *ih, int v, int code) {
        if (tid < NSLOT) {
            ih[tid] = v;
            if (tid % PHALO == 0) ih[200 + tid / PHALO] = code;
        }
    };
    // LDS-DMA of the live halo rows (256 B each): 4 slots per wave instruction, 16 lanes per slot; empty slots are skipped
    auto dma_halo = [&](const int32_t *ih) {
        for (int q = wid; q < NSLOT / 4; q += NWV) {
            const int slot = q * 4 + (lane >> 4);
            const int row = ih[slot];
            if (row >= 0)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(a.feat + (int64_t)row * C + 4 * l15),
                                                 (__attribute__((address_space(3))) void *)(halo + q * 4 * C), 16, 0, 0);
        }
    };
    // depthwise 3x3 + GELU of one group from the staged halo rows: thread (cell = tid >> 3, channels 8 (tid & 7) .. +7); cell =
    // 8 j + 4 r + c of piece j (2 x 4), whose halo is 4 x 6
    auto conv_tile = [&](const int32_t *ih, int buf) {
        const int cell = tid >> 3, cg = (tid & 7) * 8, hb = (cell >> 3) * PHALO, cy = (cell >> 2) & 1, cx = cell & 3;
        float acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = b9s[cg + c];
#pragma unroll
        for (int rr = 0; rr < 3; ++rr)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int slot = hb + (cy + rr) * PW + cx + k;
                if (ih[slot] >= 0) {                              // a zero tap leaves the accumulator unchanged exactly
                    const f32x4 v0 = *reinterpret_cast<const f32x4 *>(halo + slot * C + cg), v1 = *reinterpret_cast<const f32x4 *>(halo + slot * C + cg + 4);
                    const f32x4 k0 = *reinterpret_cast<const f32x4 *>(w9s + (rr * 3 + k) * C + cg), k1 = *reinterpret_cast<const f32x4 *>(w9s + (rr * 3 + k) * C + cg + 4);
#pragma unroll
                    for (int c = 0; c < 4; ++c) { acc[c] = fmaf(v0[c], k0[c], acc[c]); acc[4 + c] = fmaf(v1[c], k1[c], acc[4 + c]); }
                }
            }
        uint32_t hi[4], lo[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float y0 = gelu_erf(acc[2 * c]), y1 = gelu_erf(acc[2 * c + 1]);
            hi[c] = pack_bf16(y0, y1);
            lo[c] = pack_bf16(y0 - __uint_as_float(hi[c] << 16), y1 - __uint_as_float(hi[c] & 0xffff0000u));
        }
        const int ch = (tid & 7) ^ ((cell >> 1) & 7);             // 16-byte chunk swizzle (as the GEMM tiles: conflict-free fragment reads)
        *reinterpret_cast<u32x4 *>(t_hi + (buf * TCELLS + cell) * C + ch * 8) = u32x4{hi[0], hi[1], hi[2], hi[3]};
        if (X3) *reinterpret_cast<u32x4 *>(t_lo + (buf * TCELLS + cell) * C + ch * 8) = u32x4{lo[0], lo[1], lo[2], lo[3]};
    };
    // the product of one 16-cell group for HALF of this wave's columns (column tiles j = HF * J/2 .. +J/2): acc[j] = bias + W t
    // (two K halves; x3: + cross terms).  Halves keep the live accumulators at 2 J registers (J = 6 x3 spilled otherwise).
    constexpr int JH = J / 2;
    auto load_t = [&](int buf, int gq, bf16x8 &th0, bf16x8 &th1, bf16x8 &tl0, bf16x8 &tl1) {
        const int row = gq * 16 + l15;
        const int c0 = (g4 ^ ((row >> 1) & 7)) * 8, c1 = ((4 + g4) ^ ((row >> 1) & 7)) * 8;
        th0 = *reinterpret_cast<const bf16x8 *>(t_hi + (buf * TCELLS + row) * C + c0);
        th1 = *reinterpret_cast<const bf16x8 *>(t_hi + (buf * TCELLS + row) * C + c1);
        if (X3) {
            tl0 = *reinterpret_cast<const bf16x8 *>(t_lo + (buf * TCELLS + row) * C + c0);
            tl1 = *reinterpret_cast<const bf16x8 *>(t_lo + (buf * TCELLS + row) * C + c1);
        }
    };
    // bias / gamma / beta are loop-invariant LDS reads: left alone, LICM hoists all 12 J of them into registers (248 VGPRs in the
    // plain build, spills in the x3 one).  An opaque copy of the base pointer per use keeps them as LDS reads.
    auto opaque = [](const float *p) { asm volatile("" : "+v"(p)); return p; };
    auto product = [&](auto hf_tag, const bf16x8 &th0, const bf16x8 &th1, const bf16x8 &tl0, const bf16x8 &tl1, f32x4 (&acc)[JH]) {
        constexpr int HF = decltype(hf_tag)::value;
        const float *pb = opaque(pbias + col0);
#pragma unroll
        for (int jj = 0; jj < JH; ++jj) {
            const int j = HF * JH + jj;
            acc[jj] = *reinterpret_cast<const f32x4 *>(pb + 4 * j);
            acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][0], th0, acc[jj], 0, 0, 0);
            acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][1], th1, acc[jj], 0, 0, 0);
            if (X3) {
                acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][0], tl0, acc[jj], 0, 0, 0);
                acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][1], tl1, acc[jj], 0, 0, 0);
                acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfl[j][0], th0, acc[jj], 0, 0, 0);
                acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfl[j][1], th1, acc[jj], 0, 0, 0);
            }
        }
    };
    // (mean, M2) of one lane group's 8 J values of a half, reduced over the four g4 lanes of the cell
    auto half_stats = [&](const f32x4 (&acc)[JH], float &mean, float &m2) {
        float s1 = 0.f;
#pragma unroll
        for (int jj = 0; jj < JH; ++jj) s1 += (acc[jj][0] + acc[jj][1]) + (acc[jj][2] + acc[jj][3]);
        s1 += __shfl_xor(s1, 16);
        s1 += __shfl_xor(s1, 32);
        mean = s1 * (1.0f / (float)(16 * JH));
        float q = 0.f;
#pragma unroll
        for (int jj = 0; jj < JH; ++jj)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float dlt = acc[jj][r] - mean; q = fmaf(dlt, dlt, q); }
        q += __shfl_xor(q, 16);
        q += __shfl_xor(q, 32);
        m2 = q;
    };

    // ---- prologue: group 0 staged synchronously, indices of group 1 in LDS ----
    if (tid < 256) { idxh[tid] = -1; idxh[256 + tid] = -1; }
    __syncthreads();
    if (g_begin >= g_end) return;
    {
        int c0, c1;
        const int i0 = load_idx(g_begin, c0);
        const int i1 = g_begin + g_step < g_end ? load_idx(g_begin + g_step, c1) : (c1 = -1, -1);
        store_idx(idxh, i0, c0);
        store_idx(idxh + 256, i1, c1);
    }
    __syncthreads();
    dma_halo(idxh);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    conv_tile(idxh, 0);
    int buf = 0;
    for (int64_t g = g_begin, it = 0; g < g_end; g += g_step, ++it) {
        __syncthreads();                                          // B1: t[buf] complete, halo buffer free, part[buf] free
        const int32_t *ih_cur = idxh + (it & 1) * 256, *ih_nx = idxh + ((it + 1) & 1) * 256;
        const bool has_nx = g + g_step < g_end, has_n2 = g + 2 * g_step < g_end;
        if (has_nx) dma_halo(ih_nx);
        // piece codes of THIS group for pass 2 (its slot of idxh is overwritten before B2): lane's cell of group gq belongs to piece
        // 2 gq + (l15 >> 3)
        int code_cur[4];
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) code_cur[gq] = ih_cur[200 + 2 * gq + (l15 >> 3)];
        int c2 = -1;
        const int i2 = has_n2 ? load_idx(g + 2 * g_step, c2) : -1;
        // ---- pass 1: per-wave (mean, M2) of every cell over this wave's 16 J columns ----
        float *pw = part + ((buf * NWV + wid) * TCELLS) * 2;
#pragma unroll 1
        for (int gq = 0; gq < 4; ++gq) {
            bf16x8 th0, th1, tl0, tl1;
            load_t(buf, gq, th0, th1, tl0, tl1);
            float ma, qa, mb, qb;
            {
                f32x4 acc[JH];
                product(std::integral_constant<int, 0>{}, th0, th1, tl0, tl1, acc);
                half_stats(acc, ma, qa);
            }
            {
                f32x4 acc[JH];
                product(std::integral_constant<int, 1>{}, th0, th1, tl0, tl1, acc);
                half_stats(acc, mb, qb);
            }
            // two equal-sized halves (Chan): mean = (ma + mb) / 2, M2 = qa + qb + (mb - ma)^2 * n / 2 with n = 8 J per half
            const float dlt = mb - ma;
            const float mw = ma + 0.5f * dlt, m2 = qa + qb + dlt * dlt * (0.5f * (float)(16 * JH));
            if (g4 == 0) { pw[(gq * 16 + l15) * 2] = mw; pw[(gq * 16 + l15) * 2 + 1] = m2; }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's halo DMA (group it+1) has landed
        __syncthreads();                                          // B2: partials complete; every wave's DMA landed; codes of group it read
        store_idx(idxh + (it & 1) * 256, i2, c2);                 // indices of group it+2 replace those of group it (visible after B1)
        if (has_nx) conv_tile(ih_nx, buf ^ 1);
        // ---- pass 2: merge the 8 partials (Chan), recompute, normalise, + table, store ----
        {
            const float *pr = part + (buf * NWV * TCELLS) * 2;
#pragma unroll 1
            for (int gq = 0; gq < 4; ++gq) {
                const int cell = gq * 16 + l15;
                const int code = gq == 0 ? code_cur[0] : gq == 1 ? code_cur[1] : gq == 2 ? code_cur[2] : code_cur[3];
                const bool in_list = code >= 0;                     // false past the end of the live list (last group only)
                const int64_t prow = in_list ? (int64_t)((code >> 3) / a.S) * TCELLS + (code & 7) * PCELLS + (cell & 7) : 0;
                // only DIRTY cells are stored (compact row buffer); a clean cell of a live piece equals its table row bit for bit
                const int2 pd = in_list ? a.piece_dirty[g * NPIECE + (cell >> 3)] : make_int2(0, 0);
                const bool valid = (pd.y >> (cell & 7)) & 1;
                const int64_t orow = pd.x + __popc((unsigned)pd.y & ((1u << (cell & 7)) - 1u));
                const float *pep = a.pe + prow * N + col0;
                f32x4 pe0[JH], pe1[JH];                            // requested up front (HBM), consumed per half
#pragma unroll
                for (int jj = 0; jj < JH; ++jj) pe0[jj] = *reinterpret_cast<const f32x4 *>(pep + 4 * jj);
#pragma unroll
                for (int jj = 0; jj < JH; ++jj) pe1[jj] = *reinterpret_cast<const f32x4 *>(pep + 4 * (JH + jj));
                float mean = pr[cell * 2], m2 = pr[cell * 2 + 1], cnt = (float)(16 * J);
#pragma unroll
                for (int w = 1; w < NWV; ++w) {
                    const float mb = pr[(w * TCELLS + cell) * 2], m2b = pr[(w * TCELLS + cell) * 2 + 1], nb = (float)(16 * J);
                    const float dlt = mb - mean, tot = cnt + nb;
                    mean += dlt * (nb / tot);
                    m2 += m2b + dlt * dlt * (cnt * nb / tot);
                    cnt = tot;
                }
                const float rstd = 1.0f / sqrtf(m2 / (float)N + a.eps);
                bf16x8 th0, th1, tl0, tl1;
                load_t(buf, gq, th0, th1, tl0, tl1);
                uint16_t *dst = a.xh + orow * N + col0;
                uint16_t *dl = OLO ? a.xl + orow * N + col0 : nullptr;
                auto half_out = [&](auto hf_tag, const f32x4 (&pe)[JH]) {
                    constexpr int HF = decltype(hf_tag)::value;
                    f32x4 acc[JH];
                    product(hf_tag, th0, th1, tl0, tl1, acc);
                    uint32_t oh[2 * JH], ol[OLO ? 2 * JH : 1];
                    const float *pg = opaque(pgam + col0), *pbt = opaque(pbet + col0);
#pragma unroll
                    for (int jj = 0; jj < JH; ++jj) {
                        const int j = HF * JH + jj;
                        const f32x4 gv = *reinterpret_cast<const f32x4 *>(pg + 4 * j), bv = *reinterpret_cast<const f32x4 *>(pbt + 4 * j);
                        float y[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) y[r] = ((acc[jj][r] - mean) * rstd) * gv[r] + bv[r] + pe[jj][r];
                        oh[2 * jj] = pack_bf16(y[0], y[1]);
                        oh[2 * jj + 1] = pack_bf16(y[2], y[3]);
                        if (OLO) {
                            ol[2 * jj] = pack_bf16(y[0] - __uint_as_float(oh[2 * jj] << 16), y[1] - __uint_as_float(oh[2 * jj] & 0xffff0000u));
                            ol[2 * jj + 1] = pack_bf16(y[2] - __uint_as_float(oh[2 * jj + 1] << 16), y[3] - __uint_as_float(oh[2 * jj + 1] & 0xffff0000u));
                        }
                    }
                    // 4 J bytes per half and lane: J/2 8-byte pieces (16-byte stores where a pair is whole)
                    static_assert(J % 2 == 0, "even J");
                    if (valid) {
#pragma unroll
                        for (int q = 0; q < 2 * JH; q += 2) {
                            *reinterpret_cast<uint2 *>(dst + 2 * (2 * HF * JH + q)) = make_uint2(oh[q], oh[q + 1]);
                            if (OLO) *reinterpret_cast<uint2 *>(dl + 2 * (2 * HF * JH + q)) = make_uint2(ol[q], ol[q + 1]);
                        }
                    }
                };
                half_out(std::integral_constant<int, 0>{}, pe0);
                half_out(std::integral_constant<int, 1>{}, pe1);
            }
        }
        buf ^= 1;
    }
}

// ---------------------------------------------------------------------------------------------------------
// fused K|V kernel: from the pillar features straight to the K|V rows of the dirty cells, without the d-wide token.
//   x   = LayerNorm(Wp t + bp) * gamma + beta + PE[e]          (vat_lidar.py:222-248; t = GELU(dwconv3x3(pillars)) in R^64)
//   K|V = W_kv x + b_kv                                          (vat_blocks.py:42, in_proj rows d .. 3d)
// LayerNorm of a linear map of t is a per-row rescale of another linear map of t:  y - mean(y) = Wc t + bc  (Wc, bc = Wp, bp with
// their means over the d outputs removed), var(y) = |Wc t + bc|^2 / d = (|R t + r0|^2 + c0) / d  with R the 64 x 64 triangular factor
// of [Wc bc], so
//   K|V = rstd (M t + m0) + T[e],   M = W_kv diag(gamma) Wc  [2d, 64],  m0 = W_kv (gamma * bc),  T[e] = W_kv (beta + PE[e]) + b_kv,
//   rstd = 1 / sqrt((|R t + r0|^2 + c0) / d + eps)
// -- exact algebra (folded once per weights version on the host, fusion.VATLiDAR._kv_fold), and the 768-deep K|V projection becomes a
// 64-deep one.  Same skeleton as k_tile_tokens (live pieces, halo by LDS-DMA, conv in LDS, W fragments in registers, dirty cells
// stored compactly); a workgroup owns ONE column half (K or V: blockIdx bit 3), the product is computed once, the "statistics pass"
// is one 16-row tile of R per wave and 16-cell group.
// ---------------------------------------------------------------------------------------------------------
struct KvArgs {
    const float *feat;            // [M, 64] pillar features
    const int32_t *idx;           // [S, H, W] pillar row or -1
    const int32_t *live_list;     // flat piece indices (t * S + s) * 8 + p
    const int2 *piece_dirty;      // per live piece: (first dirty-row number, dirty mask)
    const int32_t *counts;        // counts[0] = live pieces
    const float *w9, *b9;         // depthwise conv [64, 9], [64]
    const uint16_t *mh, *ml;      // M [2 N, 64] bf16 hi / lo
    const float *m0;              // [2 N]
    const uint16_t *rh, *rl;      // R [64, 64] bf16 hi / lo
    const float *r0;              // [64]
    float c0, inv_d, eps;
    const float *te;              // T [H*W (tile-major), 2 N] fp32
    int S, H, W;
    uint16_t *out;                // K|V rows [dirty rows, 2 N] bf16
};

template <int J, bool X3>
__global__ void __launch_bounds__(512) k_tile_kv(KvArgs a) {
    constexpr int N = 128 * J, C = 64, NWV = 8;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    // LDS map
    uint16_t *t_hi = reinterpret_cast<uint16_t *>(smem);                      // [2][64][64] bf16, 128-byte rows, chunk-swizzled
    uint16_t *t_lo = t_hi + 2 * TCELLS * C;                                   // [2][64][64]
    float *halo = reinterpret_cast<float *>(t_lo + 2 * TCELLS * C);           // [192][64] fp32 pillar rows of the 8 halos (live slots only)
    int32_t *idxh = reinterpret_cast<int32_t *>(halo + NSLOT * C);            // [2][256]: 192 halo indices + 8 piece codes at [200..207]
    float *part = reinterpret_cast<float *>(idxh + 2 * 256);                  // [2][4 row tiles of R][64 cells]
    float *pbias = part + 2 * 4 * TCELLS;                                     // [N] m0 of this half
    float *w9s = pbias + N;                                                   // [9][64]
    float *b9s = w9s + 9 * C;                                                 // [64]
    float *r0s = b9s + C;                                                     // [64]
    uint16_t *r_hi = reinterpret_cast<uint16_t *>(r0s + C);                   // [64][64] bf16 (row-major, fragment reads are 16 B)
    uint16_t *r_lo = r_hi + C * C;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l15 = lane & 15, g4 = lane >> 4;
    const int tw = a.W / TS;
    const int n_live = a.counts[0];                             // live pieces
    const int64_t n_groups = ((int64_t)n_live + NPIECE - 1) / NPIECE;

    // work order as k_tile_tokens (each XCD one contiguous eighth of the list, its workgroups interleaved); the two column halves of
    // a group run on the same XCD (block id bit 3, or bit 0 on a grid that is not a multiple of 16)
    const bool x8 = gridDim.x >= 16 && gridDim.x % 16 == 0;
    const int nxcd = x8 ? 8 : 1;
    const int xcd = x8 ? (int)blockIdx.x & 7 : 0;
    const int half = x8 ? ((int)blockIdx.x >> 3) & 1 : (int)blockIdx.x & 1;
    const int wg_r = x8 ? (int)blockIdx.x >> 4 : (int)blockIdx.x >> 1, wg_R = x8 ? (int)gridDim.x >> 4 : ((int)gridDim.x + 1) >> 1;
    const int64_t per_x = (n_groups + nxcd - 1) / nxcd;
    const int64_t x_begin = (int64_t)xcd * per_x, x_end = x_begin + per_x < n_groups ? x_begin + per_x : n_groups;
    const int64_t g_begin = x_begin + wg_r, g_end = x_end, g_step = wg_R;
    const int ncol0 = half * N;                                  // this workgroup's first output column

    for (int e = tid; e < N; e += 512) pbias[e] = a.m0[ncol0 + e];
    for (int e = tid; e < 9 * C; e += 512) w9s[e] = a.w9[(e % C) * 9 + e / C];
    if (tid < C) { b9s[tid] = a.b9 ? a.b9[tid] : 0.f; r0s[tid] = a.r0[tid]; }
    for (int e = tid; e < C * C / 8; e += 512) {
        reinterpret_cast<u32x4 *>(r_hi)[e] = reinterpret_cast<const u32x4 *>(a.rh)[e];
        if (X3) reinterpret_cast<u32x4 *>(r_lo)[e] = reinterpret_cast<const u32x4 *>(a.rl)[e];
    }

    // M fragments (A operand) in registers: lane (m = l15, kc = g4) holds M[ncol0 + n(m, j)][8 kc .. +7] and [32 + 8 kc .. +7]
    bf16x8 wf[J][2], wfl[X3 ? J : 1][2];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int n = ncol0 + 16 * J * wid + 4 * J * (l15 >> 2) + 4 * j + (l15 & 3);
        wf[j][0] = *reinterpret_cast<const bf16x8 *>(a.mh + (int64_t)n * C + 8 * g4);
        wf[j][1] = *reinterpret_cast<const bf16x8 *>(a.mh + (int64_t)n * C + 32 + 8 * g4);
        if (X3) {
            wfl[j][0] = *reinterpret_cast<const bf16x8 *>(a.ml + (int64_t)n * C + 8 * g4);
            wfl[j][1] = *reinterpret_cast<const bf16x8 *>(a.ml + (int64_t)n * C + 32 + 8 * g4);
        }
    }
    const int col0 = 16 * J * wid + 4 * J * g4;                  // this lane's first column inside the half (4 J consecutive ones)

    auto load_idx = [&](int64_t g, int &code_out) -> int {
        code_out = -1;
        if (tid >= NSLOT) return -1;
        const int j = tid / PHALO, hc = tid - j * PHALO;
        const int64_t k = g * NPIECE + j;
        if (k >= n_live) return -1;
        const int code = a.live_list[k];
        code_out = code;
        const int p = code & 7, ts = code >> 3, t = ts / a.S, sc = ts - t * a.S;
        int y0, x0;
        piece_origin(t, p, tw, y0, x0);
        const int gy = y0 - 1 + hc / PW, gx = x0 - 1 + hc % PW;
        return (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) ? a.idx[((int64_t)sc * a.H + gy) * a.W + gx] : -1;
    };
    auto store_idx = [&](int32_t *ih, int v, int code) {
        if (tid < NSLOT) {
            ih[tid] = v;
            if (tid % PHALO == 0) ih[200 + tid / PHALO] = code;
        }
    };
    auto dma_halo = [&](const int32_t *ih) {
        for (int q = wid; q < NSLOT / 4; q += NWV) {
            const int slot = q * 4 + (lane >> 4);
            const int row = ih[slot];
            if (row >= 0)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(a.feat + (int64_t)row * C + 4 * l15),
                                                 (__attribute__((address_space(3))) void *)(halo + q * 4 * C), 16, 0, 0);
        }
    };
    // depthwise 3x3 + GELU: the SAME tap order and fmaf chain as k_tile_tokens / k_dwconv3x3_gelu
    auto conv_tile = [&](const int32_t *ih, int buf) {
        const int cell = tid >> 3, cg = (tid & 7) * 8, hb = (cell >> 3) * PHALO, cy = (cell >> 2) & 1, cx = cell & 3;
        float acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = b9s[cg + c];
#pragma unroll
        for (int rr = 0; rr < 3; ++rr)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int slot = hb + (cy + rr) * PW + cx + k;
                if (ih[slot] >= 0) {
                    const f32x4 v0 = *reinterpret_cast<const f32x4 *>(halo + slot * C + cg), v1 = *reinterpret_cast<const f32x4 *>(halo + slot * C + cg + 4);
                    const f32x4 k0 = *reinterpret_cast<const f32x4 *>(w9s + (rr * 3 + k) * C + cg), k1 = *reinterpret_cast<const f32x4 *>(w9s + (rr * 3 + k) * C + cg + 4);
#pragma unroll
                    for (int c = 0; c < 4; ++c) { acc[c] = fmaf(v0[c], k0[c], acc[c]); acc[4 + c] = fmaf(v1[c], k1[c], acc[4 + c]); }
                }
            }
        uint32_t hi[4], lo[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float y0 = gelu_erf(acc[2 * c]), y1 = gelu_erf(acc[2 * c + 1]);
            hi[c] = pack_bf16(y0, y1);
            lo[c] = pack_bf16(y0 - __uint_as_float(hi[c] << 16), y1 - __uint_as_float(hi[c] & 0xffff0000u));
        }
        const int ch = (tid & 7) ^ ((cell >> 1) & 7);
        *reinterpret_cast<u32x4 *>(t_hi + (buf * TCELLS + cell) * C + ch * 8) = u32x4{hi[0], hi[1], hi[2], hi[3]};
        if (X3) *reinterpret_cast<u32x4 *>(t_lo + (buf * TCELLS + cell) * C + ch * 8) = u32x4{lo[0], lo[1], lo[2], lo[3]};
    };
    constexpr int JH = J / 2;
    static_assert(J % 2 == 0, "even J");
    auto load_t = [&](int buf, int gq, bf16x8 &th0, bf16x8 &th1, bf16x8 &tl0, bf16x8 &tl1) {
        const int row = gq * 16 + l15;
        const int c0 = (g4 ^ ((row >> 1) & 7)) * 8, c1 = ((4 + g4) ^ ((row >> 1) & 7)) * 8;
        th0 = *reinterpret_cast<const bf16x8 *>(t_hi + (buf * TCELLS + row) * C + c0);
        th1 = *reinterpret_cast<const bf16x8 *>(t_hi + (buf * TCELLS + row) * C + c1);
        if (X3) {
            tl0 = *reinterpret_cast<const bf16x8 *>(t_lo + (buf * TCELLS + row) * C + c0);
            tl1 = *reinterpret_cast<const bf16x8 *>(t_lo + (buf * TCELLS + row) * C + c1);
        }
    };
    auto opaque = [](const float *p) { asm volatile("" : "+v"(p)); return p; };
    auto product = [&](auto hf_tag, const bf16x8 &th0, const bf16x8 &th1, const bf16x8 &tl0, const bf16x8 &tl1, f32x4 (&acc)[JH]) {
        constexpr int HF = decltype(hf_tag)::value;
        const float *pb = opaque(pbias + col0);
#pragma unroll
        for (int jj = 0; jj < JH; ++jj) {
            const int j = HF * JH + jj;
            acc[jj] = *reinterpret_cast<const f32x4 *>(pb + 4 * j);
            acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][0], th0, acc[jj], 0, 0, 0);
            acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][1], th1, acc[jj], 0, 0, 0);
            if (X3) {
                acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][0], tl0, acc[jj], 0, 0, 0);
                acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][1], tl1, acc[jj], 0, 0, 0);
                acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfl[j][0], th0, acc[jj], 0, 0, 0);
                acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfl[j][1], th1, acc[jj], 0, 0, 0);
            }
        }
    };

    // ---- prologue: group 0 staged synchronously, indices of the next group in LDS ----
    if (tid < 256) { idxh[tid] = -1; idxh[256 + tid] = -1; }
    __syncthreads();
    if (g_begin >= g_end) return;
    {
        int c0, c1;
        const int i0 = load_idx(g_begin, c0);
        const int i1 = g_begin + g_step < g_end ? load_idx(g_begin + g_step, c1) : (c1 = -1, -1);
        store_idx(idxh, i0, c0);
        store_idx(idxh + 256, i1, c1);
    }
    __syncthreads();
    dma_halo(idxh);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    conv_tile(idxh, 0);
    int buf = 0;
    for (int64_t g = g_begin, it = 0; g < g_end; g += g_step, ++it) {
        __syncthreads();                                          // B1: t[buf] complete, halo buffer free, part[buf] free
        const int32_t *ih_cur = idxh + (it & 1) * 256, *ih_nx = idxh + ((it + 1) & 1) * 256;
        const bool has_nx = g + g_step < g_end, has_n2 = g + 2 * g_step < g_end;
        if (has_nx) dma_halo(ih_nx);
        int code_cur[4];
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) code_cur[gq] = ih_cur[200 + 2 * gq + (l15 >> 3)];
        int c2 = -1;
        const int i2 = has_n2 ? load_idx(g + 2 * g_step, c2) : -1;
        // ---- |R t + r0|^2 per cell: wave w takes the 16-row tile w & 3 of R for the two 16-cell groups 2 (w >> 2), 2 (w >> 2) + 1 ----
        {
            const int rt = wid & 3;
            const uint16_t *rp = r_hi + (16 * rt + l15) * C + 8 * g4, *rpl = r_lo + (16 * rt + l15) * C + 8 * g4;
            const bf16x8 ra0 = *reinterpret_cast<const bf16x8 *>(rp), ra1 = *reinterpret_cast<const bf16x8 *>(rp + 32);
            bf16x8 rl0 = ra0, rl1 = ra1;
            if (X3) { rl0 = *reinterpret_cast<const bf16x8 *>(rpl); rl1 = *reinterpret_cast<const bf16x8 *>(rpl + 32); }
            const f32x4 rinit = *reinterpret_cast<const f32x4 *>(r0s + 16 * rt + 4 * g4);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int gq = 2 * (wid >> 2) + u;
                bf16x8 th0, th1, tl0, tl1;
                load_t(buf, gq, th0, th1, tl0, tl1);
                f32x4 v = rinit;
                v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ra0, th0, v, 0, 0, 0);
                v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ra1, th1, v, 0, 0, 0);
                if (X3) {
                    v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ra0, tl0, v, 0, 0, 0);
                    v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ra1, tl1, v, 0, 0, 0);
                    v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rl0, th0, v, 0, 0, 0);
                    v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rl1, th1, v, 0, 0, 0);
                }
                float sq = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
                sq += __shfl_xor(sq, 16);
                sq += __shfl_xor(sq, 32);
                if (g4 == 0) part[(buf * 4 + rt) * TCELLS + gq * 16 + l15] = sq;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's halo DMA (next group) has landed
        __syncthreads();                                          // B2: partial sums complete; every wave's DMA landed; codes of this group read
        store_idx(idxh + (it & 1) * 256, i2, c2);
        // ---- product, rescale, + table, store.  The table rows (T[key], 2 x 4 J bytes per lane and 16-cell group) and the piece's dirty
        // word are requested ONE 16-cell group ahead: group 0's before the conv of the next work item, group q + 1's before group q's
        // MFMAs -- with the requests issued where they were used, the four round trips per work item were the kernel's critical path
        {
            const float *pr = part + buf * 4 * TCELLS;
            auto cell_of = [&](int gq) { return gq * 16 + l15; };
            auto code_of = [&](int gq) { return gq == 0 ? code_cur[0] : gq == 1 ? code_cur[1] : gq == 2 ? code_cur[2] : code_cur[3]; };
            auto request = [&](int gq, f32x4 (&te)[2 * JH], int2 &pd) {
                const int cell = cell_of(gq), code = code_of(gq);
                const bool in_list = code >= 0;
                const int64_t prow = in_list ? (int64_t)((code >> 3) / a.S) * TCELLS + (code & 7) * PCELLS + (cell & 7) : 0;
                pd = in_list ? a.piece_dirty[g * NPIECE + (cell >> 3)] : make_int2(0, 0);
                const float *tep = a.te + prow * (2 * N) + ncol0 + col0;
#pragma unroll
                for (int jj = 0; jj < 2 * JH; ++jj) te[jj] = *reinterpret_cast<const f32x4 *>(tep + 4 * jj);
            };
            auto emit = [&](int gq, const f32x4 (&te)[2 * JH], const int2 pd) {
                const int cell = cell_of(gq);
                const bool valid = (pd.y >> (cell & 7)) & 1;
                const int64_t orow = pd.x + __popc((unsigned)pd.y & ((1u << (cell & 7)) - 1u));
                const float ss = (pr[cell] + pr[TCELLS + cell]) + (pr[2 * TCELLS + cell] + pr[3 * TCELLS + cell]) + a.c0;
                const float rstd = 1.0f / sqrtf(ss * a.inv_d + a.eps);
                bf16x8 th0, th1, tl0, tl1;
                load_t(buf, gq, th0, th1, tl0, tl1);
                uint16_t *dst = a.out + orow * (2 * N) + ncol0 + col0;
                auto half_out = [&](auto hf_tag) {
                    constexpr int HF = decltype(hf_tag)::value;
                    f32x4 acc[JH];
                    product(hf_tag, th0, th1, tl0, tl1, acc);
                    uint32_t oh[2 * JH];
#pragma unroll
                    for (int jj = 0; jj < JH; ++jj) {
                        const f32x4 tv = te[HF * JH + jj];
                        oh[2 * jj] = pack_bf16(acc[jj][0] * rstd + tv[0], acc[jj][1] * rstd + tv[1]);
                        oh[2 * jj + 1] = pack_bf16(acc[jj][2] * rstd + tv[2], acc[jj][3] * rstd + tv[3]);
                    }
                    if (valid) {
#pragma unroll
                        for (int q = 0; q < 2 * JH; q += 2)
                            *reinterpret_cast<uint2 *>(dst + 2 * (2 * HF * JH + q)) = make_uint2(oh[q], oh[q + 1]);
                    }
                };
                half_out(std::integral_constant<int, 0>{});
                half_out(std::integral_constant<int, 1>{});
            };
            f32x4 te_a[2 * JH], te_b[2 * JH];
            int2 pd_a, pd_b;
            request(0, te_a, pd_a);
            if (has_nx) conv_tile(ih_nx, buf ^ 1);
            request(1, te_b, pd_b);
            emit(0, te_a, pd_a);
            request(2, te_a, pd_a);
            emit(1, te_b, pd_b);
            request(3, te_b, pd_b);
            emit(2, te_a, pd_a);
            emit(3, te_b, pd_b);
        }
        buf ^= 1;
    }
}

// ---------------------------------------------------------------------------------------------------------
// The same computation as k_tile_kv in two launches (the default): k_conv_rows produces, per DIRTY cell and in compact row order, the
// conv token t (bf16 hi + lo, 256 B), rstd and the cell's key; k_kv_rows is then a plain 64-deep projection over contiguous 64-row
// tiles -- no halo round trip, no conv, no statistics pass and no dirty masks in the MFMA kernel, one barrier per tile, and the conv
// runs once instead of once per column half.  (k_tile_kv: 5.7 ms per 32 scenes, 51 % of its wave cycles waiting.)
// ---------------------------------------------------------------------------------------------------------
struct ConvArgs {
    const float *feat;            // [M, 64] pillar features
    const int32_t *idx;           // [S, H, W] pillar row or -1
    const int32_t *live_list;     // flat piece indices (t * S + s) * 8 + p
    const int2 *piece_dirty;      // per live piece: (first dirty-row number, dirty mask)
    const int32_t *counts;        // counts[0] = live pieces
    const float *w9, *b9;         // depthwise conv [64, 9], [64]
    const uint16_t *rh, *rl;      // R [64, 64] bf16 hi / lo (rl may be null: plain operands)
    const float *r0;              // [64]
    float c0, inv_d, eps;
    int S, H, W;
    uint16_t *th, *tl;            // out: t rows [dirty rows, 64] bf16 hi / lo (tl null: plain)
    float *rstd;                  // out: [dirty rows]
    int32_t *key;                 // out: [dirty rows] the cell's row in the table T (tile-major key index)
};

// The loop's vector-memory loads as inline asm.  The compiler's wait pass does not count them, and that is the point: with an LDS-DMA
// outstanding it waits vmcnt(0) at the first use of any load it does count and at every __syncthreads(), which put eight full drains
// into a tile of k_kv_rows and a drain per barrier into k_conv_rows.  Every load of such a loop is therefore issued here, every wait is
// a vm_wait<N>() placed by hand in the kernel, and a destination register is handed to the compiler (landed()) only behind the wait
// that retires it.  Vector-memory operations complete in issue order, so vmcnt(N) retires everything but the newest N.
typedef int i32x2 __attribute__((ext_vector_type(2)));
template <int N> __device__ __forceinline__ void vm_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int OFF> __device__ __forceinline__ void vm_load16(f32x4 &d, const void *p) {       // early clobber: d never overlaps the address pair
    asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=&v"(d) : "v"(p), "n"(OFF) : "memory");
}
__device__ __forceinline__ void vm_load8(i32x2 &d, const void *p) { asm volatile("global_load_dwordx2 %0, %1, off" : "=&v"(d) : "v"(p) : "memory"); }
template <class T> __device__ __forceinline__ void vm_load4(T &d, const void *p) {
    static_assert(sizeof(T) == 4, "one dword");
    asm volatile("global_load_dword %0, %1, off" : "=&v"(d) : "v"(p) : "memory");
}
// 16 B per lane global -> LDS at the wave-uniform LDS byte address `dst` + 16 lane (M0 is the compiler's: saved and restored)
__device__ __forceinline__ void vm_dma16(const void *src, uint32_t dst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
}
// volatile asm statements keep their order: behind a vm_wait this makes every later use of x a use of the landed value
template <class T> __device__ __forceinline__ void landed(T &x) { asm volatile("" : "+v"(x)); }
template <int... I, class F> __device__ __forceinline__ void static_for(std::integer_sequence<int, I...>, F &&f) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F> __device__ __forceinline__ void static_for(F &&f) { static_for(std::make_integer_sequence<int, N>{}, f); }
// workgroup barrier without the memory drain of __syncthreads(): LDS traffic of this wave complete, vector memory left in flight
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// A workgroup walks its groups (ordinal o = 0, 1, ... : group blockIdx.x + o gridDim.x) as a five-deep software pipeline.  One pass of
// the loop (`it`) holds, in issue order:
//     halo DMA of ordinal it + 2          (its index words reached LDS a pass ago; the second halo buffer lets it fly for a whole pass)
//     index words of ordinal it + 3       (one dword per halo slot; the piece codes they depend on are in the LDS ring since a pass ago)
//     codes + dirty entries of it + 4     (8 ints + 8 int2, fetched once per group into the ring -- not per thread before each use)
//     rstd / key stores of ordinal it     (wave 7; sums from `part`, row numbers from the ring)
//     conv of ordinal it + 1, t stores    (halo landed and index words visible since the barrier that ended the previous pass)
//     barrier B1                          (t complete)
//     |R t + r0|^2 of ordinal it + 1      (R fragments are loop-invariant per wave: registers, not LDS)
//     vm_wait<0>                          (the pass's ONE wait: DMA, index words and ring entries have had the conv and the MFMA batch to
//                                          land, so what it exposes is the tail of one round trip, not three or four in a row; it also
//                                          retires the pass's stores, the youngest of which are a MFMA batch old)
//     index words / ring entries -> LDS, barrier B2
// Nothing the loop loads is counted by the compiler (inline asm), the barriers are raw, and its stores are never waited for by the
// compiler, so the one wait is the only drain.  Every asm load is issued and retired inside one pass and by every thread (clamped
// address, result discarded where it does not apply): no destination register is live across the back edge or merged under a branch.
template <bool X3>
__global__ void __launch_bounds__(512) k_conv_rows(ConvArgs a) {
    constexpr int C = 64, NWV = 8, RING = 8;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint16_t *t_hi = reinterpret_cast<uint16_t *>(smem);                      // [64][64] bf16, chunk-swizzled (B operand of the R tiles)
    uint16_t *t_lo = t_hi + TCELLS * C;
    float *halo = reinterpret_cast<float *>(t_lo + TCELLS * C);               // [2][192][64] fp32
    int32_t *idxh = reinterpret_cast<int32_t *>(halo + 2 * NSLOT * C);        // [2][256] halo index words of two ordinals
    int32_t *mcode = idxh + 2 * 256;                                          // [RING][8] piece codes (-1: no piece)
    i32x2 *mdirty = reinterpret_cast<i32x2 *>(mcode + RING * NPIECE);         // [RING][8] (first dirty-row number, dirty mask)
    float *part = reinterpret_cast<float *>(mdirty + RING * NPIECE);          // [4][64]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l15 = lane & 15, g4 = lane >> 4;
    const int tw = a.W / TS;
    const int n_live = a.counts[0];
    const int64_t n_groups = ((int64_t)n_live + NPIECE - 1) / NPIECE;
    const int64_t g_begin = blockIdx.x, g_step = gridDim.x;
    if (g_begin >= n_groups) return;
    const int n_my = (int)((n_groups - g_begin + g_step - 1) / g_step);       // ordinals 0 .. n_my - 1 exist; later ones are empty

    // conv weights and bias: a thread convolves the same 8 channels (tid & 7) in every group -- 72 + 8 registers instead of 288 B of LDS
    // reads per thread and group (half of the conv's LDS traffic was weights)
    float wk[9][8], bk[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int ch = (tid & 7) * 8 + c;
        bk[c] = a.b9 ? a.b9[ch] : 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) wk[k][c] = a.w9[ch * 9 + k];
    }
    // R: wave w multiplies the 16-row tile w & 3 in every group -- its four fragments and its slice of r0 stay in registers
    const int rt = wid & 3;
    bf16x8 ra0, ra1, rl0, rl1;
    {
        const uint16_t *rp = a.rh + (16 * rt + l15) * C + 8 * g4;
        ra0 = *reinterpret_cast<const bf16x8 *>(rp);
        ra1 = *reinterpret_cast<const bf16x8 *>(rp + 32);
        rl0 = ra0; rl1 = ra1;
        if (X3) {
            const uint16_t *rpl = a.rl + (16 * rt + l15) * C + 8 * g4;
            rl0 = *reinterpret_cast<const bf16x8 *>(rpl);
            rl1 = *reinterpret_cast<const bf16x8 *>(rpl + 32);
        }
    }
    f32x4 rinit = *reinterpret_cast<const f32x4 *>(a.r0 + 16 * rt + 4 * g4);

    // ring entry of piece j of ordinal o: is there such a piece, and where
    auto piece_k = [&](int o, int j, bool &ok) -> int64_t {
        const int64_t grp = g_begin + (int64_t)o * g_step, k = grp * NPIECE + j;
        ok = o < n_my && k < n_live;
        return ok ? k : 0;
    };
    // this thread's halo slot of ordinal o (its codes are in the ring): offset of its index word in a.idx; !ok: no such slot, or outside the BEV
    auto idx_off = [&](int o, bool &ok) -> int64_t {
        ok = false;
        if (tid >= NSLOT) return 0;
        const int j = tid / PHALO, hc = tid - j * PHALO;
        const int code = mcode[(o & (RING - 1)) * NPIECE + j];
        if (code < 0) return 0;
        const int p = code & 7, ts = code >> 3, t = ts / a.S, sc = ts - t * a.S;
        int y0, x0;
        piece_origin(t, p, tw, y0, x0);
        const int gy = y0 - 1 + hc / PW, gx = x0 - 1 + hc % PW;
        if (gy < 0 || gy >= a.H || gx < 0 || gx >= a.W) return 0;
        ok = true;
        return ((int64_t)sc * a.H + gy) * a.W + gx;
    };
    const uint32_t lds_halo = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) float *)halo);
    auto dma_halo = [&](const int32_t *ih, int hbuf) {
        for (int q = wid; q < NSLOT / 4; q += NWV) {
            const int row = ih[q * 4 + (lane >> 4)];
            const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_halo + (uint32_t)((hbuf * NSLOT + q * 4) * C * 4));
            if (row >= 0) vm_dma16(a.feat + (int64_t)row * C + 4 * l15, dst);
        }
    };
    // depthwise 3x3 + GELU (the tap order and fmaf chain of k_dwconv3x3_gelu); the dirty cells' tokens also leave for HBM right here
    auto conv_tile = [&](const int32_t *ih, const float *hl, int o) {
        const int cell = tid >> 3, cg = (tid & 7) * 8, hb = (cell >> 3) * PHALO, cy = (cell >> 2) & 1, cx = cell & 3;
        float acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = bk[c];
#pragma unroll
        for (int rr = 0; rr < 3; ++rr)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int slot = hb + (cy + rr) * PW + cx + k;
                if (ih[slot] >= 0) {
                    const f32x4 v0 = *reinterpret_cast<const f32x4 *>(hl + slot * C + cg), v1 = *reinterpret_cast<const f32x4 *>(hl + slot * C + cg + 4);
                    const float *kk = wk[rr * 3 + k];
#pragma unroll
                    for (int c = 0; c < 4; ++c) { acc[c] = fmaf(v0[c], kk[c], acc[c]); acc[4 + c] = fmaf(v1[c], kk[4 + c], acc[4 + c]); }
                }
            }
        uint32_t hi[4], lo[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float y0 = gelu_erf(acc[2 * c]), y1 = gelu_erf(acc[2 * c + 1]);
            hi[c] = pack_bf16(y0, y1);
            lo[c] = pack_bf16(y0 - __uint_as_float(hi[c] << 16), y1 - __uint_as_float(hi[c] & 0xffff0000u));
        }
        const int ch = (tid & 7) ^ ((cell >> 1) & 7);
        *reinterpret_cast<u32x4 *>(t_hi + cell * C + ch * 8) = u32x4{hi[0], hi[1], hi[2], hi[3]};
        if (X3) *reinterpret_cast<u32x4 *>(t_lo + cell * C + ch * 8) = u32x4{lo[0], lo[1], lo[2], lo[3]};
        const int m = (o & (RING - 1)) * NPIECE + (cell >> 3);
        if (mcode[m] >= 0) {
            const i32x2 pd = mdirty[m];
            if ((pd.y >> (cell & 7)) & 1) {
                const int64_t orow = pd.x + __popc((unsigned)pd.y & ((1u << (cell & 7)) - 1u));
                *reinterpret_cast<u32x4 *>(a.th + orow * C + cg) = u32x4{hi[0], hi[1], hi[2], hi[3]};
                if (X3) *reinterpret_cast<u32x4 *>(a.tl + orow * C + cg) = u32x4{lo[0], lo[1], lo[2], lo[3]};
            }
        }
    };
    // |R t + r0|^2 per cell: wave w takes the 16-row tile w & 3 of R for the 16-cell groups 2 (w >> 2), 2 (w >> 2) + 1
    auto row_sums = [&]() {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int gq = 2 * (wid >> 2) + u;
            const int row = gq * 16 + l15;
            const int c0 = (g4 ^ ((row >> 1) & 7)) * 8, c1 = ((4 + g4) ^ ((row >> 1) & 7)) * 8;
            const bf16x8 th0 = *reinterpret_cast<const bf16x8 *>(t_hi + row * C + c0), th1 = *reinterpret_cast<const bf16x8 *>(t_hi + row * C + c1);
            f32x4 v = rinit;
            v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ra0, th0, v, 0, 0, 0);
            v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ra1, th1, v, 0, 0, 0);
            if (X3) {
                const bf16x8 tl0 = *reinterpret_cast<const bf16x8 *>(t_lo + row * C + c0), tl1 = *reinterpret_cast<const bf16x8 *>(t_lo + row * C + c1);
                v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ra0, tl0, v, 0, 0, 0);
                v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ra1, tl1, v, 0, 0, 0);
                v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rl0, th0, v, 0, 0, 0);
                v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rl1, th1, v, 0, 0, 0);
            }
            float sq = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
            sq += __shfl_xor(sq, 16);
            sq += __shfl_xor(sq, 32);
            if (g4 == 0) part[rt * TCELLS + gq * 16 + l15] = sq;
        }
    };
    // rstd and key of ordinal o's dirty cells: the last wave, one cell per lane (waves 0..2 already carry the index-word addresses)
    auto finish_rows = [&](int o) {
        if (wid != NWV - 1) return;
        const int cell = lane, m = (o & (RING - 1)) * NPIECE + (cell >> 3);
        const int code = mcode[m];
        if (code < 0) return;
        const i32x2 pd = mdirty[m];
        if ((pd.y >> (cell & 7)) & 1) {
            const int64_t orow = pd.x + __popc((unsigned)pd.y & ((1u << (cell & 7)) - 1u));
            const float ss = (part[cell] + part[TCELLS + cell]) + (part[2 * TCELLS + cell] + part[3 * TCELLS + cell]) + a.c0;
            a.rstd[orow] = 1.0f / sqrtf(ss * a.inv_d + a.eps);
            a.key[orow] = ((code >> 3) / a.S) * TCELLS + (code & 7) * PCELLS + (cell & 7);
        }
    };

    // ---- prologue (once per workgroup, plain loads and full barriers): ring entries of ordinals 0..3, index words of 0..2, halos of 0 and 1,
    // conv and row sums of ordinal 0
    if (tid < 4 * NPIECE) {
        bool ok;
        const int64_t k = piece_k(tid >> 3, tid & 7, ok);
        const int code = a.live_list[k];
        const int2 pd = a.piece_dirty[k];
        mcode[tid] = ok ? code : -1;
        mdirty[tid] = ok ? i32x2{pd.x, pd.y} : i32x2{0, 0};
    }
    __syncthreads();
    {
        bool k0, k1, k2;
        const int64_t o0 = idx_off(0, k0), o1 = idx_off(1, k1), o2 = idx_off(2, k2);
        const int i0 = a.idx[o0], i1 = a.idx[o1], i2 = a.idx[o2];
        if (tid < 256) { idxh[tid] = k0 ? i0 : -1; idxh[256 + tid] = k1 ? i1 : -1; }
        __syncthreads();
        dma_halo(idxh, 0);
        dma_halo(idxh + 256, 1);
        vm_wait<0>();                                             // both halos; the R fragments and conv weights (the compiler's own loads end here)
        landed(ra0); landed(ra1); landed(rl0); landed(rl1); landed(rinit);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            landed(bk[c]);
#pragma unroll
            for (int k = 0; k < 9; ++k) landed(wk[k][c]);
        }
        __syncthreads();
        conv_tile(idxh, halo, 0);
        __syncthreads();
        row_sums();
        if (tid < 256) idxh[tid] = k2 ? i2 : -1;                  // ordinal 2 takes over ordinal 0's words
        __syncthreads();
    }
    for (int it = 0; it < n_my; ++it) {
        // here: `part` holds ordinal it; halo[(it + 1) & 1] holds ordinal it + 1; index words of it + 1, it + 2 and ring entries up to it + 3 are in LDS
        const int cur = it & 1, nx = cur ^ 1;
        const bool has_nx = it + 1 < n_my;
        dma_halo(idxh + cur * 256, cur);                          // ordinal it + 2 into the buffer that the conv of ordinal it left before B2
        bool ok_i, ok_m;
        const int64_t off_i = idx_off(it + 3, ok_i);
        const int64_t k_m = piece_k(it + 4, tid & 7, ok_m);
        int iw, mc;
        i32x2 md;
        vm_load4(iw, a.idx + off_i);
        vm_load4(mc, a.live_list + k_m);
        vm_load8(md, a.piece_dirty + k_m);
        finish_rows(it);
        if (has_nx) conv_tile(idxh + nx * 256, halo + nx * NSLOT * C, it + 1);
        lds_barrier();                                            // B1: t complete; `part` read
        if (has_nx) row_sums();
        vm_wait<0>();                                             // retires this pass's DMA, index words, ring entries and stores
        landed(iw); landed(mc); landed(md);
        if (tid < 256) idxh[nx * 256 + tid] = ok_i ? iw : -1;     // ordinal it + 3 takes over ordinal it + 1's words (its conv is behind B1)
        if (tid < NPIECE) {
            const int m = ((it + 4) & (RING - 1)) * NPIECE + tid;
            mcode[m] = ok_m ? mc : -1;
            mdirty[m] = ok_m ? md : i32x2{0, 0};
        }
        lds_barrier();                                            // B2: `part`, every wave's DMA, the index words and the ring entries are visible
    }
}

struct KvRowArgs {
    const uint16_t *th, *tl;      // t rows [n, 64] bf16 hi / lo
    const float *rstd;            // [n]
    const int32_t *key;           // [n]
    const int32_t *n_rows;        // device-side row count
    const uint16_t *mh, *ml;      // M [2 N, 64] bf16 hi / lo
    const float *m0;              // [2 N]
    const float *te;              // T [keys, 2 N] fp32
    uint16_t *out;                // K|V rows [n, 2 N] bf16 (the K half as IEEE fp16 when k_fp16)
    int k_fp16;
};

// TH: the table T is IEEE fp16 (its values are bounded by the fold; the rounding, 2^-12, disappears under the bf16 rounding of the result):
// half the L2 traffic of the kernel's largest stream.  A lane then owns 8 consecutive columns per PAIR of column tiles, so one 16-byte
// request still covers a full 64-byte line per cell.
template <int J, bool X3, bool TH>
__global__ void __launch_bounds__(512) k_kv_rows(KvRowArgs a) {
    constexpr int N = 128 * J, C = 64, JH = J / 2;
    static_assert(J % 2 == 0, "even J");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint16_t *t_hi = reinterpret_cast<uint16_t *>(smem);                      // [2][64][64] bf16, chunk-swizzled, filled by LDS-DMA
    uint16_t *t_lo = t_hi + 2 * TCELLS * C;
    float *pbias = reinterpret_cast<float *>(t_lo + 2 * TCELLS * C);          // [N] m0 of this half
    // output staging: the MFMA layout gives a lane 4 columns of one row per column tile -- stored directly that is 8 bytes per lane,
    // 32 contiguous bytes per row and request, and the store path was 2.1 of the kernel's 4.4 ms.  The 16 x N block of a 16-row
    // group goes through LDS instead (rows padded by 16 B: the 16 rows of a request would otherwise share their banks) and leaves as
    // 1-KiB wave stores along the rows.  Two buffers: group q + 1 is written while group q is being read out.
    constexpr int SROW = N + 8;
    uint16_t *sbuf = reinterpret_cast<uint16_t *>(pbias + N);                 // [2][16][SROW] bf16
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l15 = lane & 15, g4 = lane >> 4;
    const int64_t n_rows = *a.n_rows;
    const int64_t n_groups = (n_rows + TCELLS - 1) / TCELLS;
    // each XCD one contiguous eighth of the rows (they are in (tile, scene) order: neighbouring tiles share rows of T), its
    // workgroups interleaved; the two column halves of a tile run on the same XCD
    const bool x8 = gridDim.x >= 16 && gridDim.x % 16 == 0;
    const int nxcd = x8 ? 8 : 1;
    const int xcd = x8 ? (int)blockIdx.x & 7 : 0;
    const int half = x8 ? ((int)blockIdx.x >> 3) & 1 : (int)blockIdx.x & 1;
    const int wg_r = x8 ? (int)blockIdx.x >> 4 : (int)blockIdx.x >> 1, wg_R = x8 ? (int)gridDim.x >> 4 : ((int)gridDim.x + 1) >> 1;
    const int64_t per_x = (n_groups + nxcd - 1) / nxcd;
    const int64_t x_begin = (int64_t)xcd * per_x, x_end = x_begin + per_x < n_groups ? x_begin + per_x : n_groups;
    const int64_t g_begin = x_begin + wg_r, g_end = x_end, g_step = wg_R;
    const int ncol0 = half * N;
    const bool as_f16 = a.k_fp16 != 0 && half == 0;             // workgroup-uniform: the K half leaves as fp16 ("mixed16")
    for (int e = tid; e < N; e += 512) pbias[e] = a.m0[ncol0 + e];

    bf16x8 wf[J][2], wfl[X3 ? J : 1][2];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        // column tile j of this wave, A row m = l15 -> column 16 j + m (fp32 T) or 32 (j / 2) + 8 (m / 4) + 4 (j % 2) + m % 4 (fp16 T)
        const int n = ncol0 + 16 * J * wid + (TH ? 32 * (j >> 1) + 8 * (l15 >> 2) + 4 * (j & 1) + (l15 & 3) : 16 * j + l15);
        wf[j][0] = *reinterpret_cast<const bf16x8 *>(a.mh + (int64_t)n * C + 8 * g4);
        wf[j][1] = *reinterpret_cast<const bf16x8 *>(a.mh + (int64_t)n * C + 32 + 8 * g4);
        if (X3) {
            wfl[j][0] = *reinterpret_cast<const bf16x8 *>(a.ml + (int64_t)n * C + 8 * g4);
            wfl[j][1] = *reinterpret_cast<const bf16x8 *>(a.ml + (int64_t)n * C + 32 + 8 * g4);
        }
    }
    // C layout: lane (cell = l15, g4) holds rows 4 g4 .. 4 g4 + 3 of every column tile, i.e. columns 16 J w + 16 j + 4 g4 + r: for a
    // fixed j the four g4 lanes of a cell cover 64 CONTIGUOUS bytes of its T row (one full line per cell and request; with 4 J
    // consecutive columns per lane every request touched 64 different lines for 16 bytes each: 5.50 -> 5.17 ms)
    const int col0 = 16 * J * wid + (TH ? 8 : 4) * g4;
    auto colj = [&](int j) { return TH ? 32 * (j >> 1) + 4 * (j & 1) : 16 * j; };      // lane's column of tile j, relative to col0
    // stage the 64 contiguous t rows of tile g: wave w moves rows 8 w .. 8 w + 7 (one 1-KiB LDS-DMA for hi, one for lo); LDS position
    // (row, chunk c) receives SOURCE chunk c ^ ((row >> 1) & 7), the swizzle the fragment reads expect.  Rows past the end are clamped.
    const uint32_t lds_t = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) uint16_t *)t_hi);
    auto stage = [&](int64_t g, int buf) {
        const int row = 8 * wid + (lane >> 3), c = lane & 7;
        int64_t r = g * TCELLS + row;
        r = r < n_rows ? r : n_rows - 1;
        const int64_t so = r * C + ((c ^ ((row >> 1) & 7)) << 3);
        const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_t + (uint32_t)((buf * TCELLS + 8 * wid) * C * 2));
        vm_dma16(a.th + so, dst);
        if (X3) vm_dma16(a.tl + so, dst + 2 * TCELLS * C * 2);        // t_lo
    };
    auto load_t = [&](int buf, int gq, bf16x8 &th0, bf16x8 &th1, bf16x8 &tl0, bf16x8 &tl1) {
        const int row = gq * 16 + l15;
        const int c0 = (g4 ^ ((row >> 1) & 7)) * 8, c1 = ((4 + g4) ^ ((row >> 1) & 7)) * 8;
        th0 = *reinterpret_cast<const bf16x8 *>(t_hi + (buf * TCELLS + row) * C + c0);
        th1 = *reinterpret_cast<const bf16x8 *>(t_hi + (buf * TCELLS + row) * C + c1);
        if (X3) {
            tl0 = *reinterpret_cast<const bf16x8 *>(t_lo + (buf * TCELLS + row) * C + c0);
            tl1 = *reinterpret_cast<const bf16x8 *>(t_lo + (buf * TCELLS + row) * C + c1);
        }
    };
    // the bias is re-read from LDS at every use (24 more live registers would not fit).  What is laundered per use is its 32-bit LDS
    // address: behind a laundered generic pointer the reads were FLAT loads, which count on vmcnt and lgkmcnt and can only be waited
    // for with zero; these are ds_read_b128 on lgkmcnt alone.
    const uint32_t lds_bias = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) float *)pbias) + 4 * col0;
    auto product = [&](auto hf_tag, const bf16x8 &th0, const bf16x8 &th1, const bf16x8 &tl0, const bf16x8 &tl1, f32x4 (&acc)[JH]) {
        constexpr int HF = decltype(hf_tag)::value;
        uint32_t pb = lds_bias;
        asm volatile("" : "+v"(pb));
#pragma unroll
        for (int jj = 0; jj < JH; ++jj) {
            const int j = HF * JH + jj;
            acc[jj] = *(const __attribute__((address_space(3))) f32x4 *)(pb + 4 * colj(j));
            acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][0], th0, acc[jj], 0, 0, 0);
            acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][1], th1, acc[jj], 0, 0, 0);
            if (X3) {
                acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][0], tl0, acc[jj], 0, 0, 0);
                acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][1], tl1, acc[jj], 0, 0, 0);
                acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfl[j][0], th0, acc[jj], 0, 0, 0);
                acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfl[j][1], th1, acc[jj], 0, 0, 0);
            }
        }
    };
    if (g_begin >= g_end) return;
    // ---- vector-memory accounting of the tile loop.  Per wave and tile, in issue order (every tile issues all of it, so the counts
    // hold on every path; the stores are the one exception, see `full`):
    //     stage(next tile)  D LDS-DMA pieces        meta(next tile)  M key / rstd dwords
    //     T1  R requests    [group 0: its wait W0]  E0  S output stores
    //     T2  R             [group 1: W1]           E1  S
    //     T3  R             [group 2: W2]           E2  S
    //     T0' R (group 0 of the NEXT tile)  [group 3: W3]  E3  S
    // Wq sits behind the MFMAs of group q and retires Tq; it is the only kind of wait in the loop, and what it leaves in flight is
    // listed where it is written.  The stage DMA and the meta loads need no wait of their own: they are older than T1, so W1 retires
    // them, three barriers before the staged rows are read (behind the next tile's first barrier) and before the keys are used (T0').
    constexpr int R = TH ? JH : J;                                // 16-byte T requests per lane and 16-row group (64 B apart)
    constexpr int S = N / 256;                                    // 16-byte output stores per lane and 16-row group
    constexpr int D = X3 ? 2 : 1;                                 // LDS-DMA pieces per wave and tile
    constexpr int M = 8;                                          // key + rstd dwords per lane and tile
    // the compiler's own loads (M, m0) are used, hence complete, before the first hand-counted one: from here on the only
    // vector-memory operations it counts are the output stores, which it never waits for
#pragma unroll
    for (int j = 0; j < J; ++j) {
        landed(wf[j][0]);
        landed(wf[j][1]);
        if (X3) { landed(wfl[j][0]); landed(wfl[j][1]); }
    }
    // the lane's four rows of a tile (row 16 q + l15): key and rstd, fetched a whole tile ahead so that the T requests never wait on them
    auto load_meta = [&](int64_t g, int (&kq)[4], float (&rq)[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int64_t r = g * TCELLS + q * 16 + l15;
            r = r < n_rows ? r : n_rows - 1;
            vm_load4(kq[q], a.key + r);
            vm_load4(rq[q], a.rstd + r);
        }
    };
    auto meta_landed = [&](int (&kq)[4], float (&rq)[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { landed(kq[q]); landed(rq[q]); }
    };
    // the lane's part of row `key` of T: R requests, raw (the fp16 form stays packed until its use)
    auto request = [&](int key, f32x4 (&te)[R]) {
        const char *tep = TH ? reinterpret_cast<const char *>(reinterpret_cast<const uint16_t *>(a.te) + (int64_t)key * (2 * N) + ncol0 + col0)
                             : reinterpret_cast<const char *>(a.te + (int64_t)key * (2 * N) + ncol0 + col0);
        static_for<R>([&](auto i) { vm_load16<64 * decltype(i)::value>(te[decltype(i)::value], tep); });
    };
    int kq[4], kn[4];
    float rq[4], rn[4];
    f32x4 te_a[R], te_b[R];
    load_meta(g_begin, kq, rq);                                   // M
    stage(g_begin, 0);                                            // D
    vm_wait<D>();                                                 // in flight: meta M, stage D.  Retires the meta loads.
    meta_landed(kq, rq);
    request(kq[0], te_a);                                         // R (T0 of the first tile)
    vm_wait<R>();                                                 // in flight: stage D, T0 R.  Retires the stage: read behind the loop's first barrier.
    int buf = 0;
    for (int64_t g = g_begin; g < g_end; g += g_step) {
        // first: no E3 of a previous tile lies between T0 and this tile's stage.  full: all 64 rows exist, so every wave issues every
        // one of its output stores; in the one partial tile a wave whose rows are all past the end branches around a store, so
        // there the waits do not count the stores (with the stores issued after all, that waits for them too: safe)
        const bool first = g == g_begin, full = (g + 1) * TCELLS <= n_rows;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                             // tile g complete for everyone (its DMA retired by W1..W3 of the previous tile, or above); everyone is done reading the other buffer
        asm volatile("" ::: "memory");
        const int64_t gn = g + g_step < g_end ? g + g_step : g;   // a workgroup's last tile stages and requests itself again: same counts, in-bounds, unused
        stage(gn, buf ^ 1);                                       // D
        load_meta(gn, kn, rn);                                    // M
        auto emit = [&](int gq, f32x4 (&te)[R], auto &&wait) {
            bf16x8 th0, th1, tl0, tl1;
            load_t(buf, gq, th0, th1, tl0, tl1);
            const float rs = gq == 0 ? rq[0] : gq == 1 ? rq[1] : gq == 2 ? rq[2] : rq[3];
            uint16_t *sb = sbuf + (gq & 1) * 16 * SROW;
            uint16_t *dst = sb + l15 * SROW + col0;
            auto half_out = [&](auto hf_tag) {
                constexpr int HF = decltype(hf_tag)::value;
                f32x4 acc[JH];
                product(hf_tag, th0, th1, tl0, tl1, acc);
                if constexpr (HF == 0) {
                    wait();                                       // W(gq): this group's T rows, requested one group ago
#pragma unroll
                    for (int i = 0; i < R; ++i) landed(te[i]);
                }
                uint32_t oh[2 * JH];
#pragma unroll
                for (int jj = 0; jj < JH; ++jj) {
                    const int j = HF * JH + jj;
                    f32x4 tv;
                    if (TH) {                                       // request j / 2 holds tiles 2 p, 2 p + 1: two packed half pairs -> four floats
                        const f16x2_t h0 = __builtin_bit_cast(f16x2_t, __float_as_uint(te[TH ? j >> 1 : 0][2 * (j & 1)]));
                        const f16x2_t h1 = __builtin_bit_cast(f16x2_t, __float_as_uint(te[TH ? j >> 1 : 0][2 * (j & 1) + 1]));
                        tv = f32x4{(float)h0[0], (float)h0[1], (float)h1[0], (float)h1[1]};
                    } else {
                        tv = te[TH ? 0 : j];
                    }
                    if (as_f16) {
                        oh[2 * jj] = pack_f16(acc[jj][0] * rs + tv[0], acc[jj][1] * rs + tv[1]);
                        oh[2 * jj + 1] = pack_f16(acc[jj][2] * rs + tv[2], acc[jj][3] * rs + tv[3]);
                    } else {
                        oh[2 * jj] = pack_bf16(acc[jj][0] * rs + tv[0], acc[jj][1] * rs + tv[1]);
                        oh[2 * jj + 1] = pack_bf16(acc[jj][2] * rs + tv[2], acc[jj][3] * rs + tv[3]);
                    }
                }
#pragma unroll
                for (int jj = 0; jj < JH; ++jj)
                    *reinterpret_cast<uint2 *>(dst + colj(HF * JH + jj)) = make_uint2(oh[2 * jj], oh[2 * jj + 1]);
            };
            half_out(std::integral_constant<int, 0>{});
            half_out(std::integral_constant<int, 1>{});
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                         // the 16 x N block is complete (raw: no memory drain)
            asm volatile("" ::: "memory");
            constexpr int UPR = N / 8;                            // 16-byte units per row
#pragma unroll
            for (int i = 0; i < S; ++i) {                         // E(gq): S stores
                const int u = (wid * S + i) * 64 + lane, row = u / UPR, c16 = u - row * UPR;
                const int64_t r = g * TCELLS + gq * 16 + row;
                if (r < n_rows)
                    *reinterpret_cast<u32x4 *>(a.out + r * (2 * N) + ncol0 + c16 * 8) = *reinterpret_cast<const u32x4 *>(sb + row * SROW + c16 * 8);
            }
        };
        // W1..W3: newer than the awaited T(q) are E(q-1) and T(q+1)
        auto wait_sr = [&]() { if (full) vm_wait<S + R>(); else vm_wait<R>(); };
        request(kq[1], te_b);                                     // T1: R
        emit(0, te_a, [&]() {
            // W0.  In flight, oldest first: T0 R (requested before group 3 of the previous tile, or above), E3 S of the previous tile
            // (a full one: this tile exists), stage D, meta M, T1 R.  Retires T0.
            if (first) vm_wait<D + M + R>(); else vm_wait<S + D + M + R>();
        });
        request(kq[2], te_a);                                     // T2: R
        emit(1, te_b, [&]() {
            wait_sr();                                            // W1.  In flight: stage D, meta M, T1 R, E0 S, T2 R.  Retires stage, meta and T1.
            meta_landed(kn, rn);
        });
        request(kq[3], te_b);                                     // T3: R
        emit(2, te_a, [&]() { wait_sr(); });                      // W2.  In flight: T2 R, E1 S, T3 R.  Retires T2.
        request(kn[0], te_a);                                     // T0 of the next tile: R, in flight across the tile boundary
        emit(3, te_b, [&]() { wait_sr(); });                      // W3.  In flight: T3 R, E2 S, T0' R.  Retires T3.
#pragma unroll
        for (int q = 0; q < 4; ++q) { kq[q] = kn[q]; rq[q] = rn[q]; }
        buf ^= 1;
    }
    vm_wait<0>();                                                 // the last tile's unused stage DMA and T0' request, and the stores
}

}  // namespace bt

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" size_t lvq_bev_tiles_workspace_bytes(int batch, int ny, int nx) {
    if (batch <= 0 || ny <= 0 || nx <= 0) return 0;
    const int64_t total = (int64_t)batch * (ny / 8) * (nx / 8) * bt::NPIECE;
    return lvq_align((size_t)2 * lvq_cdiv(total, bt::CNT_BLOCK) * sizeof(int32_t)) + lvq_align((size_t)total) + 512;   // (live pieces, dirty rows) per counting block + one mask byte per piece
}

extern "C" int lvq_bev_tiles(const int32_t *idx_map, int batch, int ny, int nx, int force_all, int row_base, int32_t *live_list,
                             int32_t *piece_dirty, int32_t *row_src, int32_t *counts, void *ws, size_t ws_bytes, lvq_stream_t stream) {
    if (batch <= 0 || ny <= 0 || nx <= 0 || row_base < 0 || !live_list || !piece_dirty || !row_src || !counts || (!idx_map && !force_all)) return LVQ_EINVAL;
    if ((ny % bt::TS) || (nx % bt::TS)) return LVQ_EUNSUPPORTED;
    const int64_t total = (int64_t)batch * (ny / bt::TS) * (nx / bt::TS) * bt::NPIECE;
    if ((int64_t)row_base + total * bt::PCELLS > 0x7fffffff || batch > 65535) return LVQ_EUNSUPPORTED;      // rows are int32
    if (((uintptr_t)row_src & 15) || ((uintptr_t)piece_dirty & 7) || ((uintptr_t)idx_map & 15)) return LVQ_EUNSUPPORTED;
    const int nb = (int)((total + bt::CNT_BLOCK - 1) / bt::CNT_BLOCK);
    LvqArena arena(ws, ws_bytes);
    int32_t *block_cnt = arena.take<int32_t>((size_t)2 * nb);
    uint8_t *masks = arena.take<uint8_t>((size_t)total);
    if (!arena.ok) return LVQ_EWORKSPACE;
    hipStream_t st = lvq_s(stream);
    hipLaunchKernelGGL(bt::k_piece_count, dim3(nb), dim3(256), 0, st, idx_map, batch, ny, nx, force_all, total, block_cnt, masks);
    hipLaunchKernelGGL(bt::k_piece_compact, dim3(nb), dim3(256), 0, st, idx_map, batch, ny, nx, force_all, total, (const int32_t *)block_cnt,
                       (const uint8_t *)masks, nb, row_base, live_list, reinterpret_cast<int2 *>(piece_dirty), row_src, counts);
    return lvq_launch_status();
}

template <int J> static int launch_tile_kv(const bt::KvArgs &a, bool x3, int64_t cap_tiles, hipStream_t st) {
    const size_t lds = (size_t)2 * 2 * bt::TCELLS * 64 * 2 + (size_t)bt::NSLOT * 64 * 4 + 2 * 256 * 4 + (size_t)2 * 4 * bt::TCELLS * 4 +
                       (size_t)128 * J * 4 + 9 * 64 * 4 + 64 * 4 + 64 * 4 + (size_t)2 * 64 * 64 * 2;
    static LvqLdsOnce once;
    if (!lvq_ensure_lds(once, {(const void *)bt::k_tile_kv<J, false>, (const void *)bt::k_tile_kv<J, true>}, lds)) return LVQ_ELAUNCH;
    int64_t grid = (int64_t)lvq_cu_count();
    if (grid > cap_tiles) grid = cap_tiles;
    grid *= 2;                                                   // two column halves (K, V) per group
    if (x3) hipLaunchKernelGGL((bt::k_tile_kv<J, true>), dim3((unsigned)grid), dim3(512), lds, st, a);
    else    hipLaunchKernelGGL((bt::k_tile_kv<J, false>), dim3((unsigned)grid), dim3(512), lds, st, a);
    return lvq_launch_status();
}

// K|V rows of the dirty cells straight from the pillar features (k_tile_kv): refine conv + GELU -> t, then
// kv = rstd (M t + m0) + T[key] with rstd = 1 / sqrt((|R t + r0|^2 + c0) / d_ln + eps).  n = d (the K and the V half are n columns each).
template <int J> static int launch_kv_rows(const bt::KvRowArgs &a, bool x3, bool t_f16, int64_t cap_tiles, hipStream_t st) {
    const size_t lds = (size_t)2 * 2 * bt::TCELLS * 64 * 2 + (size_t)128 * J * 4 + (size_t)2 * 16 * (128 * J + 8) * 2;
    static LvqLdsOnce once;
    if (lds > 64 * 1024 && !lvq_ensure_lds(once, {(const void *)bt::k_kv_rows<J, false, false>, (const void *)bt::k_kv_rows<J, true, false>,
                                                   (const void *)bt::k_kv_rows<J, false, true>, (const void *)bt::k_kv_rows<J, true, true>}, lds))
        return LVQ_ELAUNCH;
    int64_t grid = (int64_t)lvq_cu_count();
    if (grid > cap_tiles) grid = cap_tiles;
    grid *= 2;                                                   // two column halves (K, V) per tile
    if (t_f16) {
        if (x3) hipLaunchKernelGGL((bt::k_kv_rows<J, true, true>), dim3((unsigned)grid), dim3(512), lds, st, a);
        else    hipLaunchKernelGGL((bt::k_kv_rows<J, false, true>), dim3((unsigned)grid), dim3(512), lds, st, a);
    } else {
        if (x3) hipLaunchKernelGGL((bt::k_kv_rows<J, true, false>), dim3((unsigned)grid), dim3(512), lds, st, a);
        else    hipLaunchKernelGGL((bt::k_kv_rows<J, false, false>), dim3((unsigned)grid), dim3(512), lds, st, a);
    }
    return lvq_launch_status();
}

// workspace of the two-launch form of lvq_bev_tile_kv: t rows (hi, lo), rstd and key of up to cap_tiles * 64 dirty rows
extern "C" size_t lvq_bev_tile_kv_workspace_bytes(int64_t cap_tiles) {
    if (cap_tiles <= 0) return 0;
    LvqSizer z;
    z.take<uint16_t>((size_t)cap_tiles * 64 * 64);
    z.take<uint16_t>((size_t)cap_tiles * 64 * 64);
    z.take<float>((size_t)cap_tiles * 64);
    z.take<int32_t>((size_t)cap_tiles * 64);
    return z.total();
}

extern "C" int lvq_bev_tile_kv(const float *pillar_feat, const int32_t *idx_map, const int32_t *live_list, const int32_t *piece_dirty,
                               const int32_t *counts, int64_t cap_tiles, int batch, int ny, int nx, int c_in, const float *w9, const float *b9,
                               const lvq_bf16 *m, const lvq_bf16 *m_lo, const float *m0, const lvq_bf16 *r, const lvq_bf16 *r_lo, const float *r0,
                               float c0, int d_ln, float eps, const void *t_tiled, int t_f16, int n, int k_fp16, lvq_bf16 *kv, void *ws,
                               size_t ws_bytes, lvq_stream_t stream) {
    if (batch <= 0 || ny <= 0 || nx <= 0 || cap_tiles <= 0 || d_ln <= 0 || !idx_map || !live_list || !piece_dirty || !counts || !w9 || !m || !m0 || !r ||
        !r0 || !t_tiled || !kv)
        return LVQ_EINVAL;
    if ((m_lo == nullptr) != (r_lo == nullptr)) return LVQ_EINVAL;
    if ((k_fp16 || t_f16) && ws == nullptr) return LVQ_EUNSUPPORTED;          // fp16 K half / fp16 table: features of the two-launch form
    if (c_in != 64 || (ny % 8) || (nx % 8) || (n % 256) || n < 256 || n > 1024) return LVQ_EUNSUPPORTED;
    if (((uintptr_t)pillar_feat | (uintptr_t)m | (uintptr_t)m_lo | (uintptr_t)r | (uintptr_t)r_lo | (uintptr_t)m0 | (uintptr_t)r0 | (uintptr_t)t_tiled |
         (uintptr_t)kv) & 15)
        return LVQ_EUNSUPPORTED;
    bt::KvArgs a;
    a.feat = pillar_feat; a.idx = idx_map; a.live_list = live_list; a.piece_dirty = reinterpret_cast<const int2 *>(piece_dirty); a.counts = counts;
    a.w9 = w9; a.b9 = b9; a.mh = m; a.ml = m_lo; a.m0 = m0; a.rh = r; a.rl = r_lo; a.r0 = r0; a.c0 = c0; a.inv_d = 1.0f / (float)d_ln; a.eps = eps;
    a.te = static_cast<const float *>(t_tiled); a.S = batch; a.H = ny; a.W = nx; a.out = kv;
    hipStream_t st = lvq_s(stream);
    const bool x3 = m_lo != nullptr;
    if (ws != nullptr) {
        // two launches: conv tokens / rstd / keys of the dirty rows, then a 64-deep projection over contiguous 64-row tiles
        LvqArena arena(ws, ws_bytes);
        uint16_t *th = arena.take<uint16_t>((size_t)cap_tiles * 64 * 64);
        uint16_t *tl = arena.take<uint16_t>((size_t)cap_tiles * 64 * 64);
        float *rstd = arena.take<float>((size_t)cap_tiles * 64);
        int32_t *key = arena.take<int32_t>((size_t)cap_tiles * 64);
        if (!arena.ok) return LVQ_EWORKSPACE;
        bt::ConvArgs c;
        c.feat = pillar_feat; c.idx = idx_map; c.live_list = live_list; c.piece_dirty = a.piece_dirty; c.counts = counts; c.w9 = w9; c.b9 = b9;
        c.rh = r; c.rl = r_lo; c.r0 = r0; c.c0 = c0; c.inv_d = a.inv_d; c.eps = eps; c.S = batch; c.H = ny; c.W = nx;
        c.th = th; c.tl = x3 ? tl : nullptr; c.rstd = rstd; c.key = key;
        // t hi + lo, two fp32 halos, index words of two groups, the 8-deep ring of piece codes and dirty entries, row-sum partials
        const size_t lds = (size_t)2 * bt::TCELLS * 64 * 2 + (size_t)2 * bt::NSLOT * 64 * 4 + 2 * 256 * 4 + (size_t)8 * bt::NPIECE * (4 + 8) +
                           (size_t)4 * bt::TCELLS * 4;
        static LvqLdsOnce once;
        if (!lvq_ensure_lds(once, {(const void *)bt::k_conv_rows<false>, (const void *)bt::k_conv_rows<true>}, lds)) return LVQ_ELAUNCH;
        int64_t grid = (int64_t)lvq_cu_count();
        const int hook = lvq_tune().conv_rows_grid;                // test hook: small inputs give a workgroup 0, 1, 2, 3 ... groups
        if (hook > 0) grid = hook < grid ? hook : grid;
        else if (grid > cap_tiles) grid = cap_tiles;
        if (x3) hipLaunchKernelGGL((bt::k_conv_rows<true>), dim3((unsigned)grid), dim3(512), lds, st, c);
        else    hipLaunchKernelGGL((bt::k_conv_rows<false>), dim3((unsigned)grid), dim3(512), lds, st, c);
        bt::KvRowArgs k;
        k.th = th; k.tl = x3 ? tl : nullptr; k.rstd = rstd; k.key = key; k.n_rows = counts + 2; k.mh = m; k.ml = m_lo; k.m0 = m0; k.te = static_cast<const float *>(t_tiled); k.out = kv; k.k_fp16 = k_fp16;
        switch (n / 128) {
            case 2: return launch_kv_rows<2>(k, x3, t_f16 != 0, cap_tiles, st);
            case 4: return launch_kv_rows<4>(k, x3, t_f16 != 0, cap_tiles, st);
            case 6: return launch_kv_rows<6>(k, x3, t_f16 != 0, cap_tiles, st);
            case 8: return launch_kv_rows<8>(k, x3, t_f16 != 0, cap_tiles, st);
            default: return LVQ_EUNSUPPORTED;
        }
    }
    switch (n / 128) {
        case 2: return launch_tile_kv<2>(a, x3, cap_tiles, st);
        case 4: return launch_tile_kv<4>(a, x3, cap_tiles, st);
        case 6: return launch_tile_kv<6>(a, x3, cap_tiles, st);
        case 8: return launch_tile_kv<8>(a, x3, cap_tiles, st);
        default: return LVQ_EUNSUPPORTED;
    }
}

// Per-scene pair list for lvq_attention_bf16_tiled_signed (see k_scene_pairs): pair_src [batch, cap_tiles, 64], pair_info [batch, 2].
extern "C" int lvq_bev_scene_pairs(const int32_t *row_src, int batch, int n_tiles, int row_base, int cap_tiles, int32_t *pair_src,
                                   int32_t *pair_info, lvq_stream_t stream) {
    if (!row_src || !pair_src || !pair_info || batch <= 0 || n_tiles <= 0 || cap_tiles <= 0 || row_base < 0) return LVQ_EINVAL;
    if (((uintptr_t)row_src & 15) || (int64_t)n_tiles * bt::TCELLS > 0x7fffffff || batch > 65535) return LVQ_EUNSUPPORTED;
    if (cap_tiles >= n_tiles && cap_tiles >= 2 && !lvq_tune().pairs_one_wg) {
        // many workgroups per scene: <= 64 chunks of whole 1024-word rounds; the chunk counts use the list's last tile slot as scratch
        const int64_t ne = (int64_t)n_tiles * bt::TCELLS;
        int64_t chunk = (ne + 63) / 64;
        chunk = (chunk + 1023) / 1024 * 1024;
        const int nch = (int)((ne + chunk - 1) / chunk);
        hipLaunchKernelGGL(bt::k_scene_pair_count, dim3(nch, batch), dim3(bt::PAIR2_NT), 0, lvq_s(stream), row_src, n_tiles, row_base, cap_tiles, (int)chunk,
                           pair_src);
        hipLaunchKernelGGL(bt::k_scene_pair_write, dim3(nch, batch), dim3(bt::PAIR2_NT), 0, lvq_s(stream), row_src, n_tiles, row_base, cap_tiles, (int)chunk,
                           nch, pair_src, pair_info);
        return lvq_launch_status();
    }
    hipLaunchKernelGGL(bt::k_scene_pairs, dim3(batch), dim3(bt::PAIR_NT), 0, lvq_s(stream), row_src, n_tiles, row_base, cap_tiles, pair_src, pair_info);
    return lvq_launch_status();
}

// Lists of the shared subtraction (see k_shared_write): list_src [batch + 1, cap_tiles, 64] (entry `batch` = the G list), list_info [batch + 1, 4].
// Workspace (scratch of the call): 64 n_tiles + 512 (batch + 1) + 512 bytes.
extern "C" int lvq_bev_shared_lists(const int32_t *row_src, int batch, int n_tiles, int row_base, int cap_tiles, int32_t *list_src, int32_t *list_info,
                                    void *ws, size_t ws_bytes, lvq_stream_t stream) {
    if (!row_src || !list_src || !list_info || batch <= 0 || n_tiles <= 0 || cap_tiles <= 0 || row_base < 0) return LVQ_EINVAL;
    if (((uintptr_t)row_src & 15) || (int64_t)n_tiles * bt::TCELLS > 0x7fffffff || batch > 65534) return LVQ_EUNSUPPORTED;
    if (cap_tiles < n_tiles) return LVQ_EUNSUPPORTED;            // the G list (<= n_tiles tiles) must always fit: the scenes' lists rely on it
    const int ne = n_tiles * bt::TCELLS;
    LvqArena arena(ws, ws_bytes);
    uint8_t *flag = arena.take<uint8_t>((size_t)ne);
    int32_t *cnt = arena.take<int32_t>((size_t)(2 * batch + 1) * 64);
    if (!arena.ok) return LVQ_EWORKSPACE;
    int64_t chunk = ((int64_t)ne + 63) / 64;
    chunk = (chunk + 1023) / 1024 * 1024;
    const int nch = (int)(((int64_t)ne + chunk - 1) / chunk);
    hipStream_t st = lvq_s(stream);
    hipLaunchKernelGGL(bt::k_shared_flags, dim3((unsigned)lvq_cdiv(ne, bt::SH_NT * 4)), dim3(bt::SH_NT), 0, st, row_src, batch, ne, row_base, flag);
    hipLaunchKernelGGL(bt::k_shared_count, dim3(nch, batch), dim3(bt::SH_NT), 0, st, row_src, flag, batch, n_tiles, row_base, (int)chunk, cnt);
    hipLaunchKernelGGL(bt::k_shared_write, dim3(nch, batch + 1), dim3(bt::SH_NT), 0, st, row_src, flag, batch, n_tiles, row_base, cap_tiles, (int)chunk,
                       nch, cnt, list_src, list_info);
    return lvq_launch_status();
}

template <int J> static int launch_tile_tokens(const bt::TokArgs &a, bool x3, bool olo, int64_t cap_tiles, hipStream_t st) {
    const size_t lds = (size_t)2 * 2 * bt::TCELLS * 64 * 2 + (size_t)bt::NSLOT * 64 * 4 + 2 * 256 * 4 + (size_t)2 * 8 * bt::TCELLS * 2 * 4 +
                       (size_t)3 * 128 * J * 4 + 9 * 64 * 4 + 64 * 4;
    static LvqLdsOnce once;
    if (!lvq_ensure_lds(once, {(const void *)bt::k_tile_tokens<J, false, false>, (const void *)bt::k_tile_tokens<J, true, false>,
                               (const void *)bt::k_tile_tokens<J, true, true>}, lds))
        return LVQ_ELAUNCH;
    int64_t grid = (int64_t)lvq_cu_count();
    if (grid > cap_tiles) grid = cap_tiles;
    if (x3 && olo) hipLaunchKernelGGL((bt::k_tile_tokens<J, true, true>), dim3((unsigned)grid), dim3(512), lds, st, a);
    else if (x3)   hipLaunchKernelGGL((bt::k_tile_tokens<J, true, false>), dim3((unsigned)grid), dim3(512), lds, st, a);
    else           hipLaunchKernelGGL((bt::k_tile_tokens<J, false, false>), dim3((unsigned)grid), dim3(512), lds, st, a);
    return lvq_launch_status();
}

extern "C" int lvq_bev_tile_tokens(const float *pillar_feat, const int32_t *idx_map, const int32_t *live_list, const int32_t *piece_dirty,
                                   const int32_t *counts, int64_t cap_tiles, int batch, int ny, int nx, int c_in, const float *w9, const float *b9, const lvq_bf16 *w,
                                   const lvq_bf16 *w_lo, const float *bias, const float *gamma, const float *beta, float eps, const float *pe_tiled,
                                   int n, lvq_bf16 *x, lvq_bf16 *x_lo, lvq_stream_t stream) {
    if (batch <= 0 || ny <= 0 || nx <= 0 || cap_tiles <= 0 || !idx_map || !live_list || !piece_dirty || !counts || !w9 || !w || !gamma || !pe_tiled || !x)
        return LVQ_EINVAL;
    if (x_lo && !w_lo) return LVQ_EINVAL;
    if (c_in != 64 || (ny % 8) || (nx % 8) || (n % 256) || n < 256 || n > 1024) return LVQ_EUNSUPPORTED;
    if (((uintptr_t)pillar_feat | (uintptr_t)w | (uintptr_t)w_lo | (uintptr_t)pe_tiled | (uintptr_t)x | (uintptr_t)x_lo | (uintptr_t)bias |
         (uintptr_t)gamma | (uintptr_t)beta) & 15)
        return LVQ_EUNSUPPORTED;
    bt::TokArgs a;
    a.feat = pillar_feat; a.idx = idx_map; a.live_list = live_list; a.piece_dirty = reinterpret_cast<const int2 *>(piece_dirty); a.counts = counts; a.w9 = w9; a.b9 = b9; a.wh = w; a.wl = w_lo;
    a.bias = bias; a.gamma = gamma; a.beta = beta; a.pe = pe_tiled; a.eps = eps; a.S = batch; a.H = ny; a.W = nx; a.xh = x; a.xl = x_lo;
    hipStream_t st = lvq_s(stream);
    const bool x3 = w_lo != nullptr, olo = x_lo != nullptr;
    switch (n / 128) {
        case 2: return launch_tile_tokens<2>(a, x3, olo, cap_tiles, st);
        case 4: return launch_tile_tokens<4>(a, x3, olo, cap_tiles, st);
        case 6: return launch_tile_tokens<6>(a, x3, olo, cap_tiles, st);
        case 8: return launch_tile_tokens<8>(a, x3, olo, cap_tiles, st);
        default: return LVQ_EUNSUPPORTED;
    }
}
