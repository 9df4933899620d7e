// csrc/sparse_head.hip -- the branch convs of VoxelNeXtHead (pcdet/models/dense_heads/voxelnext_head.py:13-47) for gfx950, wave64: every
// branch of every task, SubMConv2d(128, 128, k) + BatchNorm1d + ReLU followed by SubMConv2d(128, out, 1, bias), in ONE launch over the N
// active rows of a 2-D sparse tensor.
//
//   k_sparse_head<NBR, SPLIT>   one workgroup = 64 rows x one task (grid: tiles x tasks), four waves, each owning 32 of the 128 intermediate
//                      columns of all 64 rows and of ALL the task's branches: acc[NBR][4][2] 16 x 16 fp32 tiles, 32 registers per branch
//                      and lane (192 for the six nuScenes branches, 256 for eight: VGPRs + AGPRs of the one wave per SIMD that
//                      __launch_bounds__(256) allows).  Per kernel offset, ascending: the tile's neighbour rows are gathered ONCE into
//                      LDS as bf16 hi (+ lo) -- k_sparse_conv's staging, 2 x 17 KB -- and every branch multiplies them with its own W_o
//                      on v_mfma_f32_16x16x32_bf16 (hi*hi + hi*lo + lo*hi in the bf16x3 form), channels ascending inside the offset,
//                      fp32 accumulation.  An offset no row of the tile has is skipped (it adds exact zeros).
//                      Then, branch by branch: scale / shift / ReLU from the accumulators into a 64 x 128 fp32 tile in the SAME LDS
//                      (33 KB: the intermediate never goes to HBM), and the last conv on the VALU: thread (row, slot) takes every
//                      fourth channel the branch owns and runs fmaf over the 128 intermediate channels in ascending order, + bias.
//   k_sparse_head_direct   num_conv = 1: there is no first conv; the fp32 feature tile itself is staged and the same dot product runs.
//
// Output: CHANNEL-major [16 * n_tasks, N] fp32 (channel 16 t + c of row i at (16 t + c) * N + i).  lvq_voxel_decode scans a task's hm
// channels over all rows (contiguous here) and gathers ~10 box channels for K rows only; the 64 rows of a tile are 64 consecutive
// floats of a channel, so the stores are whole 256-byte lines.  Channels no branch owns are written as zeros.
//
// Determinism: no atomics; a row's bits depend on its own neighbours only -- not on its tile, its position, N or the other scenes (a
// 16-row MFMA tile without the offset is skipped, a row without it contributes zeros; both change no bit).
#include "common.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

namespace {

constexpr int HEAD_C = 128;            // SHARED_CONV_CHANNEL
constexpr int TASK_C = 16;             // output channels of a task
constexpr int MAX_TASKS = 16;
constexpr int MAX_BR = 8;
constexpr int TILE_M = 64;
constexpr int PITCH = HEAD_C + 8;      // bf16 elements of a staged row (16-byte aligned rows, conflict-free b128 reads)
constexpr int MPITCH = HEAD_C + 4;     // floats of an intermediate row
constexpr int LDS_BYTES = 2 * TILE_M * PITCH * 2 > TILE_M * MPITCH * 4 ? 2 * TILE_M * PITCH * 2 : TILE_M * MPITCH * 4;

struct HeadTasks {                     // by value in the kernel arguments
    int n_br[MAX_TASKS];
    int owner[MAX_TASKS][TASK_C];      // branch that owns output channel c, -1: nobody
};

// out[16 t + c][row] = bias + sum_k mid[row][k] * w_last[16 t + c][k], k ascending, for the channels of task t that `br` owns (br < 0:
// every owned channel).  Thread = (row tid & 63, slot tid >> 6): the slot is wave-uniform, so the weights are uniform loads.
__device__ __forceinline__ void last_conv(const float *mid, const HeadTasks &tk, int t, int br, const float *__restrict__ w_last,
                                          const float *__restrict__ bias, int64_t tile0, int64_t n, float *__restrict__ out) {
    const int row = threadIdx.x & 63, slot = threadIdx.x >> 6;
    int seen = 0;
    for (int c = 0; c < TASK_C; ++c) {
        const int own = tk.owner[t][c];
        if (br < 0 ? own < 0 : own != br) continue;
        if ((seen++ & 3) != slot) continue;
        const float *wr = w_last + (int64_t)(t * TASK_C + c) * HEAD_C;
        const float4 *m4 = reinterpret_cast<const float4 *>(mid + row * MPITCH);
        float s = 0.f;
#pragma unroll 8
        for (int k4 = 0; k4 < HEAD_C / 4; ++k4) {
            const float4 m = m4[k4];
            s = fmaf(m.x, wr[4 * k4], s);
            s = fmaf(m.y, wr[4 * k4 + 1], s);
            s = fmaf(m.z, wr[4 * k4 + 2], s);
            s = fmaf(m.w, wr[4 * k4 + 3], s);
        }
        if (tile0 + row < n) out[(int64_t)(t * TASK_C + c) * n + tile0 + row] = s + bias[t * TASK_C + c];
    }
}

__device__ __forceinline__ void zero_unowned(const HeadTasks &tk, int t, int64_t tile0, int64_t n, float *__restrict__ out) {
    const int tid = threadIdx.x;
    if (tid >= TILE_M || tile0 + tid >= n) return;
    for (int c = 0; c < TASK_C; ++c)
        if (tk.owner[t][c] < 0) out[(int64_t)(t * TASK_C + c) * n + tile0 + tid] = 0.f;
}

template <int NBR, bool SPLIT>
__global__ void __launch_bounds__(256)
k_sparse_head(const float *__restrict__ feat, int64_t n, const int32_t *__restrict__ nbr, int kvol, HeadTasks tk, int br_stride,
              const lvq_bf16 *__restrict__ w_hi, const lvq_bf16 *__restrict__ w_lo, const float *__restrict__ scale,
              const float *__restrict__ shift, const float *__restrict__ w_last, const float *__restrict__ bias, float *__restrict__ out) {
    constexpr int MT = TILE_M / 16, NT = 2, KS = HEAD_C / 32;
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];
    __shared__ int s_nb2[2][TILE_M];                       // by offset parity, as in k_sparse_conv
    uint16_t *a_hi = reinterpret_cast<uint16_t *>(smem), *a_lo = a_hi + TILE_M * PITCH;
    float *mid = reinterpret_cast<float *>(smem);

    const int64_t tile0 = (int64_t)blockIdx.x * TILE_M;
    const int t = blockIdx.y, n_br = tk.n_br[t];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int col0 = wid * NT * 16;                        // of this wave

    f32x4 acc[NBR][MT][NT];
#pragma unroll
    for (int br = 0; br < NBR; ++br)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[br][mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int o = 0; o < kvol; ++o) {
        int *s_nb = s_nb2[o & 1];
        int r = -1;
        if (tid < TILE_M && tile0 + tid < n) {
            r = nbr ? nbr[(tile0 + tid) * kvol + o] : (int)(tile0 + tid);
            if (r < 0 || r >= n) r = -1;
        }
        if (tid < TILE_M) s_nb[tid] = r;
        if (!__syncthreads_or(r >= 0)) continue;           // no row of the tile has this offset (uniform; also fences the LDS tile)
        // gather, once for all branches: four channels per thread and step, a row's channels on consecutive lanes
        constexpr int QPR = HEAD_C / 4;
#pragma unroll
        for (int e0 = 0; e0 < TILE_M * QPR; e0 += 256) {
            const int e = e0 + tid;
            const int row = e / QPR, c4 = (e % QPR) * 4;
            const int src = s_nb[row];
            float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
            if (src >= 0) f = *reinterpret_cast<const float4 *>(feat + (int64_t)src * HEAD_C + c4);
            const float v[4] = {f.x, f.y, f.z, f.w};
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
        // a 16-row tile none of whose rows has the offset is skipped (its LDS rows are zeros)
        bool live[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) live[mt] = __ballot(s_nb[mt * 16 + l15] >= 0) != 0ull;
#pragma unroll
        for (int br = 0; br < NBR; ++br) {
            if (br >= n_br) continue;                      // (uniform)
            const int64_t wofs = ((((int64_t)t * br_stride + br) * kvol + o) * HEAD_C + col0 + l15) * HEAD_C + 8 * lq;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                bf16x8 bh[NT], bl[NT];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    bh[nt] = *reinterpret_cast<const bf16x8 *>(w_hi + wofs + (int64_t)nt * 16 * HEAD_C + ks * 32);
                    bl[nt] = SPLIT ? *reinterpret_cast<const bf16x8 *>(w_lo + wofs + (int64_t)nt * 16 * HEAD_C + ks * 32) : bh[nt];
                }
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    if (!live[mt]) continue;
                    const int arow = (mt * 16 + l15) * PITCH + 8 * lq + ks * 32;
                    const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(&a_hi[arow]);
                    bf16x8 al = ah;
                    if (SPLIT) al = *reinterpret_cast<const bf16x8 *>(&a_lo[arow]);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        acc[br][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[nt], acc[br][mt][nt], 0, 0, 0);
                        if (SPLIT) {
                            acc[br][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl[nt], acc[br][mt][nt], 0, 0, 0);
                            acc[br][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh[nt], acc[br][mt][nt], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }
    // the branches' epilogues and last convs.  Accumulator element j of lane l is (row 4 (l >> 4) + j, column l & 15) of a 16 x 16 tile.
#pragma unroll
    for (int br = 0; br < NBR; ++br) {
        if (br >= n_br) continue;                          // (uniform)
        __syncthreads();                                   // the staged tile / the previous branch's intermediate has been read
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col = col0 + nt * 16 + l15;
            const int64_t so = ((int64_t)t * br_stride + br) * HEAD_C + col;
            const float sc = scale[so], sh = shift[so];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = acc[br][mt][nt][j] * sc + sh;
                    mid[(mt * 16 + lq * 4 + j) * MPITCH + col] = v > 0.f ? v : 0.f;
                }
        }
        __syncthreads();
        last_conv(mid, tk, t, br, w_last, bias, tile0, n, out);
    }
    zero_unowned(tk, t, tile0, n, out);
}

// num_conv = 1: the last conv reads the features themselves
__global__ void __launch_bounds__(256)
k_sparse_head_direct(const float *__restrict__ feat, int64_t n, HeadTasks tk, const float *__restrict__ w_last,
                     const float *__restrict__ bias, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float mid[TILE_M * MPITCH];
    const int64_t tile0 = (int64_t)blockIdx.x * TILE_M;
    const int t = blockIdx.y, tid = threadIdx.x;
    constexpr int QPR = HEAD_C / 4;
#pragma unroll
    for (int e0 = 0; e0 < TILE_M * QPR; e0 += 256) {
        const int e = e0 + tid;
        const int row = e / QPR, c4 = (e % QPR) * 4;
        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tile0 + row < n) f = *reinterpret_cast<const float4 *>(feat + (tile0 + row) * HEAD_C + c4);
        *reinterpret_cast<float4 *>(&mid[row * MPITCH + c4]) = f;
    }
    __syncthreads();
    for (int br = 0; br < tk.n_br[t]; ++br) last_conv(mid, tk, t, br, w_last, bias, tile0, n, out);
    zero_unowned(tk, t, tile0, n, out);
}

template <bool SPLIT, typename... Args> int launch_head(int max_br, dim3 grid, hipStream_t st, Args... args) {
    if (max_br <= 4) hipLaunchKernelGGL((k_sparse_head<4, SPLIT>), grid, dim3(256), 0, st, args...);
    else if (max_br <= 6) hipLaunchKernelGGL((k_sparse_head<6, SPLIT>), grid, dim3(256), 0, st, args...);
    else hipLaunchKernelGGL((k_sparse_head<8, SPLIT>), grid, dim3(256), 0, st, args...);
    return lvq_launch_status();
}

}  // namespace

extern "C" int lvq_sparse_head(const float *feat, int64_t n, int c_in, const int32_t *nbr, int k_vol, int n_tasks, const int32_t *task_n_br,
                               int br_stride, const int32_t *chan_owner, int task_c, int num_conv, const lvq_bf16 *w_hi, const lvq_bf16 *w_lo,
                               const float *scale, const float *shift, const float *w_last, const float *bias, float *out,
                               lvq_stream_t stream) {
    if (n < 0 || c_in <= 0 || k_vol <= 0 || n_tasks <= 0 || br_stride <= 0 || task_c <= 0 || !task_n_br || !chan_owner) return LVQ_EINVAL;
    if (num_conv != 1 && num_conv != 2) return LVQ_EINVAL;
    if (c_in != HEAD_C || (k_vol != 1 && k_vol != 9) || n_tasks > MAX_TASKS || br_stride > MAX_BR || task_c > TASK_C) return LVQ_EUNSUPPORTED;
    HeadTasks tk;
    int max_br = 0;
    for (int t = 0; t < n_tasks; ++t) {
        const int nb = task_n_br[t];
        if (nb <= 0) return LVQ_EINVAL;
        if (nb > MAX_BR) return LVQ_EUNSUPPORTED;
        if (nb > br_stride) return LVQ_EINVAL;
        tk.n_br[t] = nb;
        max_br = nb > max_br ? nb : max_br;
        for (int c = 0; c < TASK_C; ++c) {
            const int own = c < task_c ? chan_owner[t * task_c + c] : -1;
            if (own >= nb) return LVQ_EINVAL;
            tk.owner[t][c] = own < 0 ? -1 : own;
        }
    }
    for (int t = n_tasks; t < MAX_TASKS; ++t) {
        tk.n_br[t] = 0;
        for (int c = 0; c < TASK_C; ++c) tk.owner[t][c] = -1;
    }
    if (!w_last || !bias || !out || (n > 0 && !feat)) return LVQ_EINVAL;
    if (num_conv == 2 && (!w_hi || !scale || !shift || (k_vol == 9 && !nbr))) return LVQ_EINVAL;
    if (((uintptr_t)feat & 15) || (num_conv == 2 && (((uintptr_t)w_hi | (uintptr_t)w_lo) & 15))) return LVQ_EUNSUPPORTED;
    if (n >= (1ll << 31)) return LVQ_EUNSUPPORTED;
    if (n == 0) return LVQ_OK;
    const dim3 grid((unsigned)lvq_cdiv(n, TILE_M), (unsigned)n_tasks);
    hipStream_t st = lvq_s(stream);
    if (num_conv == 1) {
        hipLaunchKernelGGL(k_sparse_head_direct, grid, dim3(256), 0, st, feat, n, tk, w_last, bias, out);
        return lvq_launch_status();
    }
    if (w_lo) return launch_head<true>(max_br, grid, st, feat, n, nbr, k_vol, tk, br_stride, w_hi, w_lo, scale, shift, w_last, bias, out);
    return launch_head<false>(max_br, grid, st, feat, n, nbr, k_vol, tk, br_stride, w_hi, w_lo, scale, shift, w_last, bias, out);
}
