// csrc/gemm.hip -- nn.Linear / 1x1-conv / MHA projections on bf16 MFMA tiles (gfx950).
//
//   C[m,n] = epi( sum_k A[m,k] * W[n,k] )      A [M,K] and W [N,K] both K-contiguous ("TN"), which is
// exactly the v_mfma_f32_16x16x32_bf16 operand shape: lane l of a wave supplies 8 consecutive k of
// row (l & 15) for A and of column (l & 15) for B, k-block (l >> 4) -- one 16-byte LDS read each, no
// transposes anywhere.  Replaces torch's F.linear under VATBlock / VATLiDAR / VATVision
// (vat_blocks.py:20-34, vat_lidar.py:88-97,117-120, vat_vision.py:118-137, build_linear.py:18-19).
//
// Structure: BMxBN tile per 256-thread workgroup (4 waves as 2x2, each (BM/2)x(BN/2) = TMxTN MFMA
// tiles), BK = 64, two LDS stages.  Global->register loads of tile t+1 are issued before the MFMAs of
// tile t and written to the other LDS stage after them (issue-early / write-late), one barrier per
// K-tile.  LDS rows are 128 B; the 16-byte chunk index is XOR-swizzled with (row>>1)&7 so that a
// ds_read_b128 lane group (rows 0-3,12-15 at chunk c and rows 4-11 at chunk c+1) hits 16 distinct
// 16-byte slots of the 256-byte bank row.
//
// Precision modes (SURVEY 7 "1e-3 in bf16"): accumulation is always fp32.  With plain bf16 operands
// the operand rounding alone (2^-9 relative) puts VATBlock outputs ~2e-3*max|out| from the fp32 CPU
// reference, outside the 1e-3 parity bar.  "bf16x3" therefore feeds each operand as hi + lo bf16 parts
// and runs three MFMA passes (hi*hi + hi*lo + lo*hi) over the same accumulators -- still bf16 MFMA
// tiles, ~2^-17 relative operand error.  It is implemented as K-segments of one loop, so both modes
// share every line of the kernel.
#include "common.h"
#include <stdlib.h>

namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

// two fp32 -> packed bf16 pair (v_cvt_pk_bf16_f32: round-to-nearest-even, NaN preserved); low half = a
__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
    bf16x2_t p = {(__bf16)a, (__bf16)b};
    return *reinterpret_cast<uint32_t *>(&p);
}

struct GemmArgs {
    const uint16_t *a[3];
    const uint16_t *w[3];
    int nseg;
    const float *bias, *residual, *rowtab;
    int64_t rowtab_rows;
    float alpha;
    int flags;
    int64_t M;
    int N, K;
    int64_t lda, ldw, ldc;
    int64_t a_bs, w_bs, c_bs;
    float *c32;
    uint16_t *c16, *c16lo;
    int ntx;            // tiles along N
    const int32_t *m_dev;   // k_gemm_256 only: the live row count lives on the device (sparse BEV stream); rows [*m_dev, M) are skipped
    int vec_epilogue;   // every C-side pointer / stride is 8-element aligned -> LDS-transposed 16-byte stores
    int stream_c;       // C (and the residual) is large and not re-read by this launch: non-temporal loads / stores
};

typedef uint32_t u32x4e __attribute__((ext_vector_type(4)));
typedef float f32x4e __attribute__((ext_vector_type(4)));

// XCD-aware tile order: workgroups b and b+8 share an XCD (and its L2).  Give each XCD a CONTIGUOUS range of
// tiles (x fastest) so the N/BN tiles that re-read one A row-panel run on one L2 (cdna_hip_programming T1,
// bijective form for any tile count).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// GLDS = 1: K % 64 == 0 fast path, tiles staged with global_load_lds_dwordx4 (LDS-DMA: no VGPRs, no ds_write
// pass).  The DMA writes lane-linear 1-KiB pieces (8 rows x 128 B), so the bank swizzle is applied to the
// per-lane SOURCE address and again on the ds_read (both-sides rule).  GLDS = 0: register staging with
// per-chunk predication for ragged K.
// NW = 4: waves 2x2, two LDS stages, one vmcnt(0)+barrier per K tile (2 workgroups per CU hide the DMA latency).
// NW = 8 (BM=256, BN=128, GLDS only): waves 4x2, THREE stages, tile t+2 is issued before tile t is consumed and the
// wait is a COUNTED vmcnt that leaves it in flight across a raw s_barrier -- ~96 KB of loads in flight per CU,
// which is what the short-K (K = 768) projections need to cover HBM latency.
template <int BM, int BN, int GLDS, int GELU, int NW>
__global__ void __launch_bounds__(NW * 64) k_gemm_bf16(GemmArgs g) {
    constexpr int BK = 64;
    constexpr int WROWS = NW / 2;                  // wave grid WROWS x 2
    constexpr int NT = NW * 64;
    constexpr int NSTAGE = (NW == 8 || (GLDS && BM == 64)) ? 3 : 2;    // 64x64 tiles serve the small latency-bound GEMMs: deeper ring
    constexpr int TM = BM / (WROWS * 16), TN = BN / 32;      // MFMA tiles per wave
    constexpr int LA = BM * 8 / NT, LB = BN * 8 / NT;        // 16-byte chunks per thread per stage
    constexpr int STAGE = (BM + BN) * 128;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    constexpr int WTM = BM / WROWS;                // rows of the wave tile
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t m0 = (int64_t)(tile / g.ntx) * BM;
    const int n0 = (tile % g.ntx) * BN;
    const int64_t z = blockIdx.z;
    const int nk = (g.K + BK - 1) / BK;
    const int n_it = nk * g.nseg;

    uint4 ra[LA], rb[LB];
    // segment bases as SGPR-resident deltas: an indexed read of the kernarg array inside the K loop is an s_load (a pending
    // scalar load forces every LDS wait to lgkmcnt(0)), and a select chain over the three loaded pointers gets turned back
    // into a private-memory lookup table by the optimiser
    const int64_t dA1 = g.a[1] - g.a[0], dA2 = g.a[2] - g.a[0], dW1 = g.w[1] - g.w[0], dW2 = g.w[2] - g.w[0];
    auto gload = [&](int it) __attribute__((always_inline)) {
        // K tiles run k-major, segment-minor: the hi and lo passes over one K tile are adjacent, so an operand that is the same in
        // two segments (A in the x2w form, A / W in bf16x3) is re-read while it is still in L2 (segment-major order streamed A
        // from HBM once per segment: 33.6 GB read for 7.3 GB of A on the live-row K|V projection, PMC FETCH_SIZE)
        const int kt = it / g.nseg, seg = it - kt * g.nseg, k0 = kt * BK;
        const uint16_t *A = (g.a[0] + (seg == 0 ? (int64_t)0 : seg == 1 ? dA1 : dA2)) + z * g.a_bs;
        const uint16_t *W = (g.w[0] + (seg == 0 ? (int64_t)0 : seg == 1 ? dW1 : dW2)) + z * g.w_bs;
#pragma unroll
        for (int i = 0; i < LA; ++i) {
            const int q = tid + NT * i, row = q >> 3, kk = k0 + (q & 7) * 8;
            const int64_t gm = m0 + row;
            ra[i] = (gm < g.M && kk < g.K) ? *reinterpret_cast<const uint4 *>(A + gm * g.lda + kk) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < LB; ++i) {
            const int q = tid + NT * i, row = q >> 3, kk = k0 + (q & 7) * 8;
            const int gn = n0 + row;
            rb[i] = (gn < g.N && kk < g.K) ? *reinterpret_cast<const uint4 *>(W + (int64_t)gn * g.ldw + kk) : make_uint4(0, 0, 0, 0);
        }
    };
    auto lstore = [&](int buf) __attribute__((always_inline)) {
        uint8_t *sa = smem + buf * STAGE, *sb = sa + BM * 128;
#pragma unroll
        for (int i = 0; i < LA; ++i) {
            const int q = tid + NT * i, row = q >> 3, ch = (q & 7) ^ ((row >> 1) & 7);
            *reinterpret_cast<uint4 *>(sa + row * 128 + ch * 16) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < LB; ++i) {
            const int q = tid + NT * i, row = q >> 3, ch = (q & 7) ^ ((row >> 1) & 7);
            *reinterpret_cast<uint4 *>(sb + row * 128 + ch * 16) = rb[i];
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // tiles are staged strictly in order, so (segment, k0) just advance (no division in the loop)
    int d_seg = 0, d_k0 = 0;
    auto stage_dma = [&](int /*it*/, int buf) __attribute__((always_inline)) {
        const int seg = d_seg, k0 = d_k0;
        if (++d_seg >= g.nseg) { d_seg = 0; d_k0 += BK; }
        const uint16_t *A = (g.a[0] + (seg == 0 ? (int64_t)0 : seg == 1 ? dA1 : dA2)) + z * g.a_bs;
        const uint16_t *W = (g.w[0] + (seg == 0 ? (int64_t)0 : seg == 1 ? dW1 : dW2)) + z * g.w_bs;
        uint8_t *sa = smem + buf * STAGE, *sb = sa + BM * 128;
        const int r8 = lane >> 3, pch = lane & 7;
#pragma unroll
        for (int i = 0; i < BM / (8 * NW); ++i) {
            const int piece = i * NW + wid, row = piece * 8 + r8;
            int64_t gm = m0 + row;
            gm = gm < g.M ? gm : g.M - 1;                    // clamped rows are never stored
            const uint16_t *src = A + gm * g.lda + k0 + ((pch ^ ((row >> 1) & 7)) << 3);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(sa + piece * 1024), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < BN / (8 * NW); ++i) {
            const int piece = i * NW + wid, row = piece * 8 + r8;
            int gn = n0 + row;
            gn = gn < g.N ? gn : g.N - 1;
            const uint16_t *src = W + (int64_t)gn * g.ldw + k0 + ((pch ^ ((row >> 1) & 7)) << 3);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(sb + piece * 1024), 16, 0, 0);
        }
    };

    auto compute = [&](int buf) __attribute__((always_inline)) {
        const uint8_t *sa = smem + buf * STAGE, *sb = sa + BM * 128;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 af[TM], bfr[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = wm * WTM + i * 16 + (lane & 15);
                const int ch = (ks * 4 + (lane >> 4)) ^ ((row >> 1) & 7);
                af[i] = *reinterpret_cast<const bf16x8 *>(sa + row * 128 + ch * 16);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int row = wn * (BN / 2) + j * 16 + (lane & 15);
                const int ch = (ks * 4 + (lane >> 4)) ^ ((row >> 1) & 7);
                bfr[j] = *reinterpret_cast<const bf16x8 *>(sb + row * 128 + ch * 16);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
    };

    if (NSTAGE == 3) {
        // Software-pipelined ring: the fragments of K-half ks+1 are read from LDS while the MFMAs of K-half ks run, and
        // the counted wait + barrier sits in the MIDDLE of the tile, so the first fragments of tile it+1 are prefetched
        // under the second MFMA cluster of tile it (the 2-barrier form left the matrix pipe idle during every read burst).
        constexpr int NLD = BM / (8 * NW) + BN / (8 * NW);       // global_load_lds per wave per stage
        auto read_frags = [&](int buf, int ks, bf16x8 (&af)[TM], bf16x8 (&bfr)[TN]) {
            const uint8_t *sa = smem + buf * STAGE, *sb = sa + BM * 128;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = wm * WTM + i * 16 + (lane & 15);
                const int ch = (ks * 4 + (lane >> 4)) ^ ((row >> 1) & 7);
                af[i] = *reinterpret_cast<const bf16x8 *>(sa + row * 128 + ch * 16);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int row = wn * (BN / 2) + j * 16 + (lane & 15);
                const int ch = (ks * 4 + (lane >> 4)) ^ ((row >> 1) & 7);
                bfr[j] = *reinterpret_cast<const bf16x8 *>(sb + row * 128 + ch * 16);
            }
        };
        auto mma = [&](bf16x8 (&af)[TM], bf16x8 (&bfr)[TN]) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        };
        stage_dma(0, 0);
        if (n_it > 1) {
            stage_dma(1, 1);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        bf16x8 a0[TM], b0[TN], a1[TM], b1[TN];
        read_frags(0, 0, a0, b0);
        // drain scalar loads before the loop (builtin, so the waitcnt pass sees it): a pending s_load in the pre-header state
        // would make every LDS wait inside the loop lgkmcnt(0) instead of a counted one
        __builtin_amdgcn_s_waitcnt(0xc07f);
        int buf = 0;
        // the last two tiles are peeled so the steady-state body is branch-free (the waitcnt pass merges states at every
        // join: with a conditional wait it falls back to lgkmcnt(0) after the prefetch reads and the overlap is lost)
        for (int it = 0; it + 2 < n_it; ++it) {
            int nb = buf + 2; nb = nb >= 3 ? nb - 3 : nb;
            const int nx = buf == 2 ? 0 : buf + 1;
            stage_dma(it + 2, nb);                             // slot last read in iteration it-1 (mid-tile barrier since)
            read_frags(buf, 1, a1, b1);
            __builtin_amdgcn_sched_barrier(0);
            mma(a0, b0);
            __builtin_amdgcn_sched_barrier(0);
            // tile it+1 landed (tile it+2 stays in flight); every LDS read of tile `it` has completed before the barrier.
            // Builtin form so the compiler's waitcnt pass knows a1/b1 are complete (gfx9 encoding: vmcnt[3:0] | expcnt<<4 |
            // lgkmcnt<<8 | vmcnt[5:4]<<14)
            __builtin_amdgcn_s_waitcnt((NLD & 15) | 0x70 | ((NLD >> 4) << 14));
            __builtin_amdgcn_s_barrier();
            read_frags(nx, 0, a0, b0);
            __builtin_amdgcn_sched_barrier(0);
            mma(a1, b1);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(0xc07f);                // a0/b0 landed under the 16 MFMAs above: free, and it keeps the
            buf = nx;                                          // compiler from placing a full lgkmcnt(0) after the NEXT reads
        }
        if (n_it > 1) {                                        // tile n_it-2: nothing left to stage, drain the DMA queue
            const int nx = buf == 2 ? 0 : buf + 1;
            read_frags(buf, 1, a1, b1);
            __builtin_amdgcn_sched_barrier(0);
            mma(a0, b0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(0x0070);
            __builtin_amdgcn_s_barrier();
            read_frags(nx, 0, a0, b0);
            __builtin_amdgcn_sched_barrier(0);
            mma(a1, b1);
            __builtin_amdgcn_sched_barrier(0);
            buf = nx;
        }
        read_frags(buf, 1, a1, b1);
        mma(a0, b0);
        mma(a1, b1);
        __builtin_amdgcn_s_barrier();      // epilogue reuses the ring as its transpose slab
    } else {
        if (GLDS) {
            stage_dma(0, 0);
        } else {
            gload(0);
            lstore(0);
        }
        __syncthreads();   // with an LDS-DMA in flight hipcc emits s_waitcnt vmcnt(0) in front of this barrier
        for (int it = 0; it < n_it; ++it) {
            const int buf = it & 1;
            if (it + 1 < n_it) {
                if (GLDS) stage_dma(it + 1, buf ^ 1); else gload(it + 1);
            }
            compute(buf);
            if (!GLDS && it + 1 < n_it) lstore(buf ^ 1);
            __syncthreads();
        }
    }

    // ---- epilogue ----
    // C/D layout of 16x16x32: lane l holds rows (l>>4)*4 + r, column l & 15 of each 16x16 tile.
    constexpr bool gelu = GELU == 1;     // template parameter: the inlined erff() is only instantiated where it is used
    constexpr bool qgelu = GELU == 2;    // LVQ_GEMM_QUICK_GELU: x sigmoid(1.702 x), a third value of the same parameter
    if (g.vec_epilogue) {
        // Transpose through a wave-private LDS slab so that every lane owns 8 CONSECUTIVE columns of one row:
        // bias / residual / table reads and all stores become 16- or 32-byte accesses (the direct layout
        // gives 2-byte bf16 stores in 32-byte row segments, which made K <= 768 GEMMs store-bound).
        constexpr int HR = WTM / 2;                      // rows per half of the wave tile (32 or 16)
        constexpr int WC = BN / 2;                       // columns of the wave tile (64 or 32)
        constexpr int LDE = WC + 4;                      // padded row (floats); (WC+4)*4 B is a multiple of 16
        constexpr int CPR = WC / 8;                      // 8-column chunks per row
        float *ep = reinterpret_cast<float *>(smem) + wid * (HR * LDE);
        static_assert(NW * HR * LDE * 4 <= NSTAGE * STAGE, "epilogue slab must fit in the staging LDS");
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
#pragma unroll
            for (int ii = 0; ii < TM / 2; ++ii)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        ep[(ii * 16 + (lane >> 4) * 4 + r) * LDE + j * 16 + (lane & 15)] = acc[hh * (TM / 2) + ii][j][r];
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll 1
            for (int p = 0; p < (HR * CPR) / 64; ++p) {     // rolled: the epilogue was 27k instructions (I-cache) fully unrolled
                const int q = p * 64 + lane, rr = q / CPR, c8 = q % CPR;
                const int64_t row = m0 + wm * WTM + hh * HR + rr;
                const int col = n0 + wn * WC + c8 * 8;
                float v[8];
                *reinterpret_cast<float4 *>(v) = *reinterpret_cast<const float4 *>(ep + rr * LDE + c8 * 8);
                *reinterpret_cast<float4 *>(v + 4) = *reinterpret_cast<const float4 *>(ep + rr * LDE + c8 * 8 + 4);
                if (row < g.M && col < g.N) {     // N % 8 == 0 in this path: a chunk is all-in or all-out
                    if (g.bias) {
                        const float4 b0 = *reinterpret_cast<const float4 *>(g.bias + col), b1 = *reinterpret_cast<const float4 *>(g.bias + col + 4);
                        v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w; v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
                    }
                    if (gelu) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = gelu_erf(v[e]);
                    }
                    if (qgelu) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = gelu_quick(v[e]);
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] *= g.alpha;
                    const int64_t o = z * g.c_bs + row * g.ldc + col;
                    if (g.residual) {
                        f32x4e r0, r1;
                        if (g.stream_c) {
                            r0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4e *>(g.residual + o));
                            r1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4e *>(g.residual + o + 4));
                        } else {
                            r0 = *reinterpret_cast<const f32x4e *>(g.residual + o);
                            r1 = *reinterpret_cast<const f32x4e *>(g.residual + o + 4);
                        }
                        v[0] += r0[0]; v[1] += r0[1]; v[2] += r0[2]; v[3] += r0[3]; v[4] += r1[0]; v[5] += r1[1]; v[6] += r1[2]; v[7] += r1[3];
                    }
                    if (g.rowtab) {
                        const float *t = g.rowtab + (row % g.rowtab_rows) * g.N + col;
                        const float4 t0 = *reinterpret_cast<const float4 *>(t), t1 = *reinterpret_cast<const float4 *>(t + 4);
                        v[0] += t0.x; v[1] += t0.y; v[2] += t0.z; v[3] += t0.w; v[4] += t1.x; v[5] += t1.y; v[6] += t1.z; v[7] += t1.w;
                    }
                    if (g.c32) {
                        if (g.stream_c) {
                            __builtin_nontemporal_store(f32x4e{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4e *>(g.c32 + o));
                            __builtin_nontemporal_store(f32x4e{v[4], v[5], v[6], v[7]}, reinterpret_cast<f32x4e *>(g.c32 + o + 4));
                        } else {
                            *reinterpret_cast<float4 *>(g.c32 + o) = *reinterpret_cast<float4 *>(v);
                            *reinterpret_cast<float4 *>(g.c32 + o + 4) = *reinterpret_cast<float4 *>(v + 4);
                        }
                    }
                    if (g.c16) {
                        const uint4 hb = make_uint4(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7]));
                        if (g.stream_c) __builtin_nontemporal_store(u32x4e{hb.x, hb.y, hb.z, hb.w}, reinterpret_cast<u32x4e *>(g.c16 + o));
                        else            *reinterpret_cast<uint4 *>(g.c16 + o) = hb;
                        if (g.c16lo) {
                            const uint4 lb = make_uint4(pack_bf16(v[0] - __uint_as_float(hb.x << 16), v[1] - __uint_as_float(hb.x & 0xffff0000u)),
                                                        pack_bf16(v[2] - __uint_as_float(hb.y << 16), v[3] - __uint_as_float(hb.y & 0xffff0000u)),
                                                        pack_bf16(v[4] - __uint_as_float(hb.z << 16), v[5] - __uint_as_float(hb.z & 0xffff0000u)),
                                                        pack_bf16(v[6] - __uint_as_float(hb.w << 16), v[7] - __uint_as_float(hb.w & 0xffff0000u)));
                            *reinterpret_cast<uint4 *>(g.c16lo + o) = lb;
                        }
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        return;
    }
    // scalar fallback (N, ldc or a pointer not 8-element aligned)
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = n0 + wn * (BN / 2) + j * 16 + (lane & 15);
            if (col >= g.N) continue;
            const float bias = g.bias ? g.bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = m0 + wm * WTM + i * 16 + (lane >> 4) * 4 + r;
                if (row >= g.M) continue;
                float v = acc[i][j][r] + bias;
                if (gelu) v = gelu_erf(v);
                if (qgelu) v = gelu_quick(v);
                v *= g.alpha;
                const int64_t o = z * g.c_bs + row * g.ldc + col;
                if (g.residual) v += g.residual[o];
                if (g.rowtab) v += g.rowtab[(row % g.rowtab_rows) * g.N + col];
                if (g.c32) g.c32[o] = v;
                if (g.c16) {
                    const uint16_t h = f32_to_bf16(v);
                    g.c16[o] = h;
                    if (g.c16lo) g.c16lo[o] = f32_to_bf16(v - bf16_to_f32(h));
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// 256x256 tile, 8 waves (2 x 4, wave tile 128 x 64), A ring of 3 x 32 KiB + W ring of 2 x 32 KiB = all 160 KiB of LDS.
// Why: with the 256x128 tile the projections are bound by the L2 -> LDS fill (ablation on M=1M, N=1536, K=768:
// the DMA + barriers alone take 3.0 of 3.15 ms), and fill bytes per MAC go as 1/BM + 1/BN -- this tile moves
// 2/3 of the bytes.  Requires M % 256 == 0, N % 256 == 0, K % 64 == 0 and the vector epilogue (no clamps, no
// predicates); everything else takes k_gemm_bf16.
// Every A byte is an HBM (or Infinity-Cache) miss while W stays in L2: aliasing all A rows onto one row took the same
// launch from 2.55 to 1.94 ms.  So the A stream is staged TWO K tiles ahead (3 slots) and the W stream one (2 slots),
// issued W-before-A so that the in-order vmcnt can wait for "tile it+1" while the newest A tile stays in flight.
// Schedule per K tile `it`, all waits after an MFMA cluster:
//   read frags(tile it, k-half 1) | 32 MFMA (k-half 0) | vmcnt(4) lgkmcnt(0), barrier -> the slots of tile it are
//   free and tile it+1 has landed | DMA W(it+2), A(it+3) | read frags(tile it+1, k-half 0) | 32 MFMA (k-half 1)
// ---------------------------------------------------------------------------------------------------------
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

// NT = streaming (non-temporal) C stores: the 256x256 projections write 128 KiB of C per workgroup, 4 MiB per round of an
// XCD's 32 CUs -- exactly its L2 -- and evict the A panels / W tiles the other workgroups are about to re-read
template <int GELU, bool NT = false>
__device__ __forceinline__ void store_chunk8(const GemmArgs &g, int64_t z, int64_t row, int col, float (&v)[8], const float *bias_regs = nullptr) {
    if (bias_regs) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += bias_regs[e];
    } else if (g.bias) {
        const float4 b0 = *reinterpret_cast<const float4 *>(g.bias + col), b1 = *reinterpret_cast<const float4 *>(g.bias + col + 4);
        v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w; v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
    }
    if (GELU == 1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = gelu_erf(v[e]);
    }
    if (GELU == 2) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = gelu_quick(v[e]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= g.alpha;
    const int64_t o = z * g.c_bs + row * g.ldc + col;
    if (g.residual) {
        const float4 r0 = *reinterpret_cast<const float4 *>(g.residual + o), r1 = *reinterpret_cast<const float4 *>(g.residual + o + 4);
        v[0] += r0.x; v[1] += r0.y; v[2] += r0.z; v[3] += r0.w; v[4] += r1.x; v[5] += r1.y; v[6] += r1.z; v[7] += r1.w;
    }
    if (g.rowtab) {
        const float *t = g.rowtab + (row % g.rowtab_rows) * g.N + col;
        const float4 t0 = *reinterpret_cast<const float4 *>(t), t1 = *reinterpret_cast<const float4 *>(t + 4);
        v[0] += t0.x; v[1] += t0.y; v[2] += t0.z; v[3] += t0.w; v[4] += t1.x; v[5] += t1.y; v[6] += t1.z; v[7] += t1.w;
    }
    if (g.c32) {
        if (NT) {
            __builtin_nontemporal_store(f32x4v{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4v *>(g.c32 + o));
            __builtin_nontemporal_store(f32x4v{v[4], v[5], v[6], v[7]}, reinterpret_cast<f32x4v *>(g.c32 + o + 4));
        } else {
            *reinterpret_cast<float4 *>(g.c32 + o) = *reinterpret_cast<float4 *>(v);
            *reinterpret_cast<float4 *>(g.c32 + o + 4) = *reinterpret_cast<float4 *>(v + 4);
        }
    }
    if (g.c16) {
        const uint4 hb = make_uint4(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7]));
        if (NT) __builtin_nontemporal_store(u32x4{hb.x, hb.y, hb.z, hb.w}, reinterpret_cast<u32x4 *>(g.c16 + o));
        else    *reinterpret_cast<uint4 *>(g.c16 + o) = hb;
        if (g.c16lo) {
            const uint4 lb = make_uint4(pack_bf16(v[0] - __uint_as_float(hb.x << 16), v[1] - __uint_as_float(hb.x & 0xffff0000u)),
                                        pack_bf16(v[2] - __uint_as_float(hb.y << 16), v[3] - __uint_as_float(hb.y & 0xffff0000u)),
                                        pack_bf16(v[4] - __uint_as_float(hb.z << 16), v[5] - __uint_as_float(hb.z & 0xffff0000u)),
                                        pack_bf16(v[6] - __uint_as_float(hb.w << 16), v[7] - __uint_as_float(hb.w & 0xffff0000u)));
            if (NT) __builtin_nontemporal_store(u32x4{lb.x, lb.y, lb.z, lb.w}, reinterpret_cast<u32x4 *>(g.c16lo + o));
            else    *reinterpret_cast<uint4 *>(g.c16lo + o) = lb;
        }
    }
}

// Measured dead end: an LDS-free epilogue (product computed transposed with W rows permuted so that a lane owns 8 + 8
// consecutive output columns and stores straight from the accumulators) is bit-correct but 4-5 % slower on the K|V projection
// (10.28 vs 9.85 ms at 16 scenes, same box): its stores cover 64 contiguous bytes per row and instruction, the LDS-transposed
// form below writes whole 128-byte lines.
// Measured dead end: a persistent form of this kernel (one workgroup per CU walking tiles, the next tile's three A tiles
// requested before the current epilogue, its W tiles after it, epilogue slab in the W ring) needs ~8 more VGPRs than the 256
// available with 128 accumulators + two fragment sets: the spills sit in the prologue / tail code and their reloads wait on
// vmcnt, i.e. on the very requests that were meant to fly under the epilogue -- 2.99 vs 2.50 ms on the K|V projection.
template <int GELU, int ANT>
__global__ void __launch_bounds__(512) k_gemm_256(GemmArgs g) {
    constexpr int BM = 256, BN = 256, BK = 64, NW = 8;
    constexpr int TM = 8, TN = 4;                   // 16x16 MFMA tiles per wave: 128 rows x 64 columns
    constexpr int ASLOT = BM * 128, WSLOT = BN * 128;          // 32 KiB each
    constexpr int WBASE = 3 * ASLOT;                // A ring: 3 slots at 0; W ring: 2 slots behind it (160 KiB in all)
    constexpr int NA = BM / (8 * NW), NWL = BN / (8 * NW);     // global_load_lds per wave per A / W tile (4, 4)
    // ANT: the A stream is loaded non-temporal (evict-first) so that it does not displace W in the 4 MiB L2 -- right when few
    // N-tiles share an A panel (K|V projection, 6 tiles: 969 -> 1021 TFLOP/s), wrong when many do (8192^3, 32 tiles: 1290 -> 1100)
    constexpr int A_CPOL = ANT ? 2 : 0;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 2, wn = wid & 3;
    // device-side row count: the grid covers the capacity, the workgroups past the live rows leave at once, and the XCD-aware
    // order is taken over the LIVE tile count (over the grid it would park all the work on the first XCDs)
    int n_act = gridDim.x;
    if (g.m_dev) {
        int64_t live = *g.m_dev;
        live = live < 0 ? 0 : (live > g.M ? g.M : live);
        n_act = (int)((live + BM - 1) / BM) * g.ntx;
        if ((int)blockIdx.x >= n_act) return;
    }
    const int tile = xcd_remap(blockIdx.x, n_act);
    const int64_t m0 = (int64_t)(tile / g.ntx) * BM;
    const int n0 = (tile % g.ntx) * BN;
    const int64_t z = blockIdx.z;
    const int nk = g.K / BK;
    const int n_it = nk * g.nseg;

    // DMA source: lane (r8, pch) of wave `wid` fetches the 16-byte chunk pch ^ swz(row) of row piece*8 + r8, piece = i*8 + wid;
    // (row >> 1) & 7 depends on (wid & 1, r8) only, so the swizzled per-lane base pointer is fixed and pieces / K tiles /
    // split segments are uniform offsets on top of it
    const int r8 = lane >> 3, pch = lane & 7;
    const int sw = (pch ^ ((((wid & 1) << 2) + (r8 >> 1)) & 7)) << 3;
    const uint16_t *pa = g.a[0] + z * g.a_bs + (m0 + wid * 8 + r8) * g.lda + sw;
    const uint16_t *pw = g.w[0] + z * g.w_bs + (int64_t)(n0 + wid * 8 + r8) * g.ldw + sw;
    const int64_t dA1 = g.a[1] - g.a[0], dA2 = g.a[2] - g.a[0], dW1 = g.w[1] - g.w[0], dW2 = g.w[2] - g.w[0];
    const int64_t a_step = 64 * g.lda, w_step = 64 * g.ldw;
    // the A stream (HBM misses: every A byte is new) runs TWO tiles ahead, the W stream (L2 hits) one; each keeps its own
    // in-order (segment, k0) cursor
    int a_seg = 0, a_k0 = 0, w_seg = 0, w_k0 = 0;
    // tile cursors: *_next() returns the source of the next tile of the stream and advances; *_piece() issues one 1-KiB
    // global_load_lds of it (pieces are issued one per MFMA row inside the K loop, never as a burst: a burst of 8 per wave x 8
    // waves back-pressures the VMEM issue port and holds up the LDS reads + MFMAs queued behind it)
    auto a_next = [&]() __attribute__((always_inline)) -> const uint16_t * {
        const uint16_t *A = pa + (a_seg == 0 ? (int64_t)0 : a_seg == 1 ? dA1 : dA2) + a_k0;
        if (++a_seg >= g.nseg) { a_seg = 0; a_k0 += BK; }      // k-major, segment-minor (see k_gemm_bf16::gload)
        return A;
    };
    auto w_next = [&]() __attribute__((always_inline)) -> const uint16_t * {
        const uint16_t *W = pw + (w_seg == 0 ? (int64_t)0 : w_seg == 1 ? dW1 : dW2) + w_k0;
        if (++w_seg >= g.nseg) { w_seg = 0; w_k0 += BK; }
        return W;
    };
    auto a_piece = [&](const uint16_t *A, int slot, int i) __attribute__((always_inline)) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(A + i * a_step),
                                         (__attribute__((address_space(3))) void *)(smem + slot * ASLOT + wid * 1024 + i * (NW * 1024)), 16, 0, A_CPOL);
    };
    auto w_piece = [&](const uint16_t *W, int slot, int i) __attribute__((always_inline)) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(W + i * w_step),
                                         (__attribute__((address_space(3))) void *)(smem + WBASE + slot * WSLOT + wid * 1024 + i * (NW * 1024)), 16, 0, 0);
    };
    auto dma_a = [&](int slot) __attribute__((always_inline)) {
        const uint16_t *A = a_next();
#pragma unroll
        for (int i = 0; i < NA; ++i) a_piece(A, slot, i);
    };
    auto dma_w = [&](int slot) __attribute__((always_inline)) {
        const uint16_t *W = w_next();
#pragma unroll
        for (int i = 0; i < NWL; ++i) w_piece(W, slot, i);
    };
    // fragment addresses: row*128 + ((ks*4 + (lane>>4)) ^ ((row>>1)&7))*16; row = base16 + (lane&15) with base16 % 16 == 0, so the
    // XOR term depends on the lane only and k-half 1 is the same address with bit 6 flipped
    const int frow = lane & 15;
    const int fx = (((lane >> 4) ^ ((frow >> 1) & 7)) << 4);
    const int fa = (wm * 128 + frow) * 128 + fx;                 // + i*2048
    const int fb = WBASE + (wn * 64 + frow) * 128 + fx;          // + j*2048
    auto read_frags = [&](int as, int ws, int ks, bf16x8 (&af)[TM], bf16x8 (&bfr)[TN]) __attribute__((always_inline)) {
        const uint8_t *sa = smem + as * ASLOT, *sb = smem + ws * WSLOT;
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const bf16x8 *>(sa + ((fa + i * 2048) ^ (ks << 6)));
#pragma unroll
        for (int j = 0; j < TN; ++j) bfr[j] = *reinterpret_cast<const bf16x8 *>(sb + ((fb + j * 2048) ^ (ks << 6)));
    };
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto mma = [&](bf16x8 (&af)[TM], bf16x8 (&bfr)[TN]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    };
    constexpr int WAIT_A = (NA & 15) | 0x70 | ((NA >> 4) << 14);           // vmcnt(NA) lgkmcnt(0): one A tile stays in flight
    constexpr int WAIT_0 = 0x0070;                                         // vmcnt(0) lgkmcnt(0)

    // queue order A0 W0 A1 W1 A2: vmcnt is in-order, so "tile t landed" = everything but the newer A tile(s) has returned
    dma_a(0); dma_w(0);
    if (n_it > 2) {
        dma_a(1); dma_w(1); dma_a(2);
        __builtin_amdgcn_s_waitcnt(((2 * NA + NWL) & 15) | 0x70 | (((2 * NA + NWL) >> 4) << 14));
    } else if (n_it > 1) {
        dma_a(1); dma_w(1);
        __builtin_amdgcn_s_waitcnt(((NA + NWL) & 15) | 0x70 | (((NA + NWL) >> 4) << 14));
    } else {
        __builtin_amdgcn_s_waitcnt(WAIT_0);
    }
    __builtin_amdgcn_s_barrier();
    bf16x8 a0[TM], b0[TN], a1[TM], b1[TN];
    read_frags(0, 0, 0, a0, b0);
    __builtin_amdgcn_s_waitcnt(0xc07f);
    int as = 0, ws = 0;
    // one K tile: k-half 1 fragments | 32 MFMA | wait + barrier (tile it+1 landed, tile it fully read) | refill the two slots
    // just drained | k-half 0 fragments of tile it+1 | 32 MFMA.  Flags are literal at every call site (branch-free bodies).
    auto k_tile = [&](bool issue_w, bool issue_a, bool a_in_flight) __attribute__((always_inline)) {
        const int an = as == 2 ? 0 : as + 1;
        read_frags(as, ws, 1, a1, b1);
        __builtin_amdgcn_sched_barrier(0);
        mma(a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        if (a_in_flight) __builtin_amdgcn_s_waitcnt(WAIT_A); else __builtin_amdgcn_s_waitcnt(WAIT_0);
        __builtin_amdgcn_s_barrier();
        const uint16_t *Wn = issue_w ? w_next() : nullptr;     // W tile it+2 (older in the queue than ...)
        const uint16_t *An = issue_a ? a_next() : nullptr;     // ... A tile it+3
        read_frags(an, ws ^ 1, 0, a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        static_assert(NWL + NA == TM, "one DMA piece per MFMA row");
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[i], b1[j], acc[i][j], 0, 0, 0);
            if (i < NWL) { if (issue_w) w_piece(Wn, ws, i); }
            else         { if (issue_a) a_piece(An, as, i - NWL); }
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);                    // a0/b0 landed under the MFMAs (the DMAs stay in flight)
        as = an; ws ^= 1;
    };
    for (int it = 0; it + 3 < n_it; ++it) k_tile(true, true, true);
    if (n_it >= 3) k_tile(true, false, true);
    if (n_it >= 2) k_tile(false, false, false);
    read_frags(as, ws, 1, a1, b1);
    // a lane stores the same 8-column chunk (lane % 8) in every pass of the epilogue: its bias values are fetched once per tile,
    // and requested here so that the load flies under the last 64 MFMAs (at the top of the epilogue it cost ~1 us per tile)
    float bv[8];
    {
        const int colb = n0 + wn * 64 + (lane % 8) * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) bv[e] = g.bias ? g.bias[colb + e] : 0.f;
    }
    mma(a0, b0);
    mma(a1, b1);
    __builtin_amdgcn_s_barrier();                              // the epilogue reuses the A ring as its transpose slab

    // ---- epilogue: 16 rows x 64 columns per wave per pass through a wave-private LDS slab, 16/32-byte stores ----
    constexpr int HR = 16, WC = 64, LDE = WC + 4, CPR = WC / 8;
    static_assert(NW * HR * LDE * 4 <= 3 * ASLOT, "epilogue slab must fit in the A ring");
    float *ep = reinterpret_cast<float *>(smem) + wid * (HR * LDE);
#pragma unroll
    for (int ii = 0; ii < TM; ++ii) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                ep[((lane >> 4) * 4 + r) * LDE + j * 16 + (lane & 15)] = acc[ii][j][r];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll 1
        for (int p = 0; p < (HR * CPR) / 64; ++p) {
            const int q = p * 64 + lane, rr = q / CPR, c8 = q % CPR;
            float v[8];
            *reinterpret_cast<float4 *>(v) = *reinterpret_cast<const float4 *>(ep + rr * LDE + c8 * 8);
            *reinterpret_cast<float4 *>(v + 4) = *reinterpret_cast<const float4 *>(ep + rr * LDE + c8 * 8 + 4);
            store_chunk8<GELU, true>(g, z, m0 + wm * 128 + ii * 16 + rr, n0 + wn * WC + c8 * 8, v, bv);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------------------------------------------------
// Row-complete GEMM with LayerNorm fused into the epilogue (VATLiDAR token path, vat_lidar.py:222-248):
//     Y = LayerNorm(A W^T + bias) * gamma + beta + post[row % post_rows]        -> bf16 (hi, lo)
// One workgroup owns 64 rows x ALL N columns (N <= 1024), so the row statistics never leave registers and the
// fp32 [M, N] intermediate (3.2 GB per 4 scenes at d = 768) is never written.  Meant for SMALL K (the 1x1 conv
// has K = C_in = 64..128): W is streamed through LDS in 32-wide K steps, single-buffered (2 workgroups per CU
// overlap); the op is bound by the bf16 store + the positional-table read, not by MFMA.
// Wave w owns rows 16w..16w+15 and all NT16 = N/16 column tiles (acc = NT16 x 4 registers).
// ---------------------------------------------------------------------------------------------------------
struct GemmLnArgs {
    const uint16_t *a[3];
    const uint16_t *w[3];
    int nseg;
    const float *bias, *gamma, *beta, *post;
    int64_t post_rows;
    float eps;
    int64_t M;
    int N, K;
    int64_t lda, ldw;
    uint16_t *y16, *y16lo;
    int scenes;       // > 0: M = scenes * post_rows with whole 64-row tiles per scene -> scene-interleaved tile order
};

template <int NT16>
__global__ void __launch_bounds__(256, (NT16 <= 48 ? 2 : 1)) k_gemm_ln(GemmLnArgs g) {
    constexpr int N = NT16 * 16;
    constexpr int WROW = 40;                         // bf16 elements per staged row (32 + 8 pad: 80-byte rows, odd x 16 B)
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint16_t *sw = reinterpret_cast<uint16_t *>(smem);          // [N][WROW]
    uint16_t *sa = sw + N * WROW;                                 // [64][WROW]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g4 = lane >> 4, l15 = lane & 15;
    // Tile order.  The positional table (post_rows x N fp32: 805 MB at 512x512x768) is the largest operand and every scene
    // re-reads all of it; walking the tiles scene-major streamed it from HBM once per scene.  Scene-interleaved order puts
    // the `scenes` workgroups that share a table tile on the SAME XCD (block ids 8 apart) back to back, so the table
    // leaves HBM once per step and the repeats are L2 hits.
    int64_t m0 = (int64_t)blockIdx.x * 64;
    if (g.scenes > 0) {
        const int x = blockIdx.x & 7, k = blockIdx.x >> 3;
        const int sc = k % g.scenes, pt = (k / g.scenes) * 8 + x;
        m0 = ((int64_t)sc * (g.post_rows >> 6) + pt) * 64;
    }
    const int nk = g.K / 32;

    f32x4 acc[NT16];
#pragma unroll
    for (int j = 0; j < NT16; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int it = 0; it < nk * g.nseg; ++it) {
        const int kt = it / g.nseg, seg = it - kt * g.nseg, k0 = kt * 32;
        const uint16_t *A = g.a[seg], *W = g.w[seg];
        // stage W[:, k0:k0+32] (N rows x 4 chunks) and A[m0:m0+64, k0:k0+32]
        // N*4 chunks / 256 threads = NT16/4 per thread, issued in batches of 4 independent loads before the LDS writes
        // (a load->store loop pays one L2 latency per iteration)
#pragma unroll
        for (int b0 = 0; b0 < NT16 / 4; b0 += 4) {
            uint4 tmp[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = tid + (b0 + u) * 256, r = e >> 2, ch = e & 3;
                if (b0 + u < NT16 / 4) tmp[u] = *reinterpret_cast<const uint4 *>(W + (int64_t)r * g.ldw + k0 + ch * 8);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = tid + (b0 + u) * 256, r = e >> 2, ch = e & 3;
                if (b0 + u < NT16 / 4) *reinterpret_cast<uint4 *>(sw + r * WROW + ch * 8) = tmp[u];
            }
        }
        {
            const int r = tid >> 2, ch = tid & 3;
            int64_t gm = m0 + r;
            gm = gm < g.M ? gm : g.M - 1;
            *reinterpret_cast<uint4 *>(sa + r * WROW + ch * 8) = *reinterpret_cast<const uint4 *>(A + gm * g.lda + k0 + ch * 8);
        }
        __syncthreads();
        const bf16x8 af = *reinterpret_cast<const bf16x8 *>(sa + (wid * 16 + l15) * WROW + g4 * 8);
#pragma unroll
        for (int j = 0; j < NT16; ++j) {
            const bf16x8 bfr = *reinterpret_cast<const bf16x8 *>(sw + (j * 16 + l15) * WROW + g4 * 8);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr, acc[j], 0, 0, 0);
        }
        __syncthreads();
    }

    // ---- bias, then LayerNorm statistics: lane (l15, g4) holds rows 4*g4 + r, columns 16 j + l15 ----
    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NT16; ++j) {
        const float b = g.bias ? g.bias[j * 16 + l15] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) { acc[j][r] += b; s[r] += acc[j][r]; }
    }
    float mean[4], rstd[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) s[r] += __shfl_xor(s[r], o);
        mean[r] = s[r] / (float)N;
        s[r] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < NT16; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) { acc[j][r] -= mean[r]; s[r] = fmaf(acc[j][r], acc[j][r], s[r]); }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) s[r] += __shfl_xor(s[r], o);
        rstd[r] = 1.0f / sqrtf(s[r] / (float)N + g.eps);
    }

    // ---- epilogue in 64-column chunks through a wave-private slab: 16 rows x 64 columns -> 16-byte stores ----
    constexpr int LDE = 68;
    float *ep = reinterpret_cast<float *>(smem) + wid * (16 * LDE);
#pragma unroll
    for (int cc = 0; cc < NT16 / 4; ++cc) {          // fully unrolled: the accumulator tiles need static register indices
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int r = 0; r < 4; ++r) ep[(g4 * 4 + r) * LDE + jj * 16 + l15] = acc[cc * 4 + jj][r] * rstd[r];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int q = p * 64 + lane, rr = q >> 3, c8 = q & 7;
            const int64_t row = m0 + wid * 16 + rr;
            const int col = cc * 64 + c8 * 8;
            float v[8];
            *reinterpret_cast<float4 *>(v) = *reinterpret_cast<const float4 *>(ep + rr * LDE + c8 * 8);
            *reinterpret_cast<float4 *>(v + 4) = *reinterpret_cast<const float4 *>(ep + rr * LDE + c8 * 8 + 4);
            if (row < g.M) {
                const float4 g0 = *reinterpret_cast<const float4 *>(g.gamma + col), g1 = *reinterpret_cast<const float4 *>(g.gamma + col + 4);
                v[0] *= g0.x; v[1] *= g0.y; v[2] *= g0.z; v[3] *= g0.w; v[4] *= g1.x; v[5] *= g1.y; v[6] *= g1.z; v[7] *= g1.w;
                if (g.beta) {
                    const float4 b0 = *reinterpret_cast<const float4 *>(g.beta + col), b1 = *reinterpret_cast<const float4 *>(g.beta + col + 4);
                    v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w; v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
                }
                if (g.post) {
                    const float *t = g.post + (row % g.post_rows) * N + col;
                    const float4 t0 = *reinterpret_cast<const float4 *>(t), t1 = *reinterpret_cast<const float4 *>(t + 4);
                    v[0] += t0.x; v[1] += t0.y; v[2] += t0.z; v[3] += t0.w; v[4] += t1.x; v[5] += t1.y; v[6] += t1.z; v[7] += t1.w;
                }
                const int64_t o = row * N + col;
                const uint4 hb = make_uint4(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7]));
                *reinterpret_cast<uint4 *>(g.y16 + o) = hb;
                if (g.y16lo) {
                    const uint4 lb = make_uint4(pack_bf16(v[0] - __uint_as_float(hb.x << 16), v[1] - __uint_as_float(hb.x & 0xffff0000u)),
                                                pack_bf16(v[2] - __uint_as_float(hb.y << 16), v[3] - __uint_as_float(hb.y & 0xffff0000u)),
                                                pack_bf16(v[4] - __uint_as_float(hb.z << 16), v[5] - __uint_as_float(hb.z & 0xffff0000u)),
                                                pack_bf16(v[6] - __uint_as_float(hb.w << 16), v[7] - __uint_as_float(hb.w & 0xffff0000u)));
                    *reinterpret_cast<uint4 *>(g.y16lo + o) = lb;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------------------------------------------------
// Row-streaming form of the same op for K = 64 (the 1x1 conv of the BEV token path), plain bf16 operands.
// The tile kernel above is latency-bound: every thread walks 24 dependent {table load -> LDS transpose -> store} steps with
// 8 waves per CU (1.4-1.6 ms for 4 x 512 x 512 rows, ~3x its HBM time).  Here
//   * W (N x 64 bf16, <= 128 KiB) is staged into LDS ONCE per workgroup (swizzled 128-byte rows); after that
//     one barrier the waves never synchronise again;
//   * the product is computed TRANSPOSED (W rows are the MFMA A operand, 16 data rows the B operand, fetched straight
//     from global): the C layout then gives each lane 4 output columns of ONE data row per tile, and with the column
//     assignment n = 64 G + 16 g + 4 t + r (g = lane >> 4, t = tile of the group, r = register) a lane owns 16 CONSECUTIVE
//     columns of its row per group of 4 tiles -- stores, table and gamma/beta reads are whole 16-byte vectors, no LDS
//     transpose;
//   * with K = 64 the product costs two MFMAs per tile, so LayerNorm is done in three passes that RECOMPUTE it
//     (mean, centred variance, output): no N-wide accumulator;
//   * a wave handles the same 16 table rows for up to SB scenes at once: the positional table (805 MB fp32 at
//     512 x 512 x 768) is read from HBM exactly once per step, into registers, whatever the caches do.
// ---------------------------------------------------------------------------------------------------------
constexpr int LNR_WAVES = 8;       // 2 waves per SIMD: ~220 VGPRs (af 32 + two table chunks 32 + packed outputs 32 + fragments); 12 waves spilled (0.93 vs 0.72 ms)
template <int NG, int SB>
__global__ void __launch_bounds__(LNR_WAVES * 64) k_gemm_ln_rows(GemmLnArgs g, int n_ptiles, int scenes, int64_t rows_per_scene) {
    constexpr int N = NG * 64;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t *sw = smem;                                         // [N][128 B], 16-byte chunk c of row n at (c ^ f(n)) * 16
    float *sbias = reinterpret_cast<float *>(smem + N * 128), *sgam = sbias + N, *sbet = sgam + N;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g4 = lane >> 4, l15 = lane & 15;
    // f(n) = bit1(n) | ((n >> 4) & 3) << 1: conflict-free for the A-operand ds_read_b128 below (rows 16 b + 4 t + r, b = l15 >> 2)
    for (int e = tid; e < N * 8; e += LNR_WAVES * 64) {
        const int row = e >> 3, ch = e & 7;
        const uint4 v = *reinterpret_cast<const uint4 *>(g.w[0] + (int64_t)row * g.ldw + ch * 8);
        const int f = ((row >> 1) & 1) | (((row >> 4) & 3) << 1);
        *reinterpret_cast<uint4 *>(sw + row * 128 + ((ch ^ f) << 4)) = v;
    }
    for (int e = tid; e < N; e += LNR_WAVES * 64) {
        sbias[e] = g.bias ? g.bias[e] : 0.f;
        sgam[e] = g.gamma[e];
        sbet[e] = g.beta ? g.beta[e] : 0.f;
    }
    __syncthreads();

    const int fsw = ((l15 >> 1) & 1) | ((l15 >> 2) << 1);
    const uint8_t *wrow = sw + (16 * (l15 >> 2) + (l15 & 3)) * 128;      // + (64 G + 4 t) * 128
    const int wc0 = (g4 ^ fsw) << 4, wc1 = ((4 + g4) ^ fsw) << 4;        // k chunks g4 and 4 + g4 of the row
    const int cofs = 16 * g4;                                            // first of this lane's 16 columns in a group
    const float inv_n = 1.0f / (float)N;

    for (int tile = blockIdx.x * LNR_WAVES + wid; tile < n_ptiles; tile += gridDim.x * LNR_WAVES) {
        const int64_t p = (int64_t)tile * 16 + l15;                      // row inside a scene (= table row)
        for (int s0 = 0; s0 < scenes; s0 += SB) {
            // B operand: 16 data rows x 64 k per scene, straight from global (lane: row l15, k = 8 g4 .. +7 and 32 + 8 g4 ..)
            bf16x8 af[SB][2];
            int64_t rows[SB];
#pragma unroll
            for (int sc = 0; sc < SB; ++sc) {
                int64_t r = (int64_t)(s0 + sc < scenes ? s0 + sc : scenes - 1) * rows_per_scene + p;
                rows[sc] = r;
                r = r < g.M ? r : g.M - 1;
                const uint16_t *src = g.a[0] + r * g.lda + 8 * g4;
                af[sc][0] = *reinterpret_cast<const bf16x8 *>(src);
                af[sc][1] = *reinterpret_cast<const bf16x8 *>(src + 32);
            }
            // ---- pass 1: mean, pass 2: centred sum of squares (both recompute z = W a + bias) ----
            float mean[SB], rstd[SB];
#pragma unroll
            for (int sc = 0; sc < SB; ++sc) mean[sc] = 0.f;
#pragma unroll 1
            for (int gt = 0; gt < NG * 4; ++gt) {
                const int G = gt >> 2, t = gt & 3;
                const uint8_t *wa = wrow + (64 * G + 4 * t) * 128;
                const bf16x8 f0 = *reinterpret_cast<const bf16x8 *>(wa + wc0), f1 = *reinterpret_cast<const bf16x8 *>(wa + wc1);
                const f32x4 bv = *reinterpret_cast<const f32x4 *>(sbias + 64 * G + cofs + 4 * t);
#pragma unroll
                for (int sc = 0; sc < SB; ++sc) {
                    f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f0, af[sc][0], bv, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f1, af[sc][1], acc, 0, 0, 0);
                    mean[sc] += (acc[0] + acc[1]) + (acc[2] + acc[3]);
                }
            }
#pragma unroll
            for (int sc = 0; sc < SB; ++sc) {
                mean[sc] += __shfl_xor(mean[sc], 16);
                mean[sc] += __shfl_xor(mean[sc], 32);
                mean[sc] *= inv_n;
                rstd[sc] = 0.f;
            }
#pragma unroll 1
            for (int gt = 0; gt < NG * 4; ++gt) {
                const int G = gt >> 2, t = gt & 3;
                const uint8_t *wa = wrow + (64 * G + 4 * t) * 128;
                const bf16x8 f0 = *reinterpret_cast<const bf16x8 *>(wa + wc0), f1 = *reinterpret_cast<const bf16x8 *>(wa + wc1);
                const f32x4 bv = *reinterpret_cast<const f32x4 *>(sbias + 64 * G + cofs + 4 * t);
#pragma unroll
                for (int sc = 0; sc < SB; ++sc) {
                    f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f0, af[sc][0], bv, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f1, af[sc][1], acc, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) { const float d = acc[r] - mean[sc]; rstd[sc] = fmaf(d, d, rstd[sc]); }
                }
            }
#pragma unroll
            for (int sc = 0; sc < SB; ++sc) {
                rstd[sc] += __shfl_xor(rstd[sc], 16);
                rstd[sc] += __shfl_xor(rstd[sc], 32);
                rstd[sc] = 1.0f / sqrtf(rstd[sc] * inv_n + g.eps);
            }
            // ---- pass 3: output, one 64-column group at a time; the table chunk is loaded once for all SB scenes ----
            // the table chunk of group G+1 is requested while group G is computed (every chunk is an HBM miss)
            f32x4 pen[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) pen[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float *ps = g.post ? g.post + (p % g.post_rows) * N + cofs : nullptr;
            if (ps) {
#pragma unroll
                for (int t = 0; t < 4; ++t) pen[t] = *reinterpret_cast<const f32x4 *>(ps + 4 * t);
            }
#pragma unroll 1
            for (int G = 0; G < NG; ++G) {
                f32x4 pe[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) pe[t] = pen[t];
                if (ps && G + 1 < NG) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) pen[t] = *reinterpret_cast<const f32x4 *>(ps + 64 * (G + 1) + 4 * t);
                }
                uint32_t out[SB][8];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const uint8_t *wa = wrow + (64 * G + 4 * t) * 128;
                    const bf16x8 f0 = *reinterpret_cast<const bf16x8 *>(wa + wc0), f1 = *reinterpret_cast<const bf16x8 *>(wa + wc1);
                    const f32x4 bv = *reinterpret_cast<const f32x4 *>(sbias + 64 * G + cofs + 4 * t);
                    const f32x4 gv = *reinterpret_cast<const f32x4 *>(sgam + 64 * G + cofs + 4 * t);
                    const f32x4 be = *reinterpret_cast<const f32x4 *>(sbet + 64 * G + cofs + 4 * t);
#pragma unroll
                    for (int sc = 0; sc < SB; ++sc) {
                        f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f0, af[sc][0], bv, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f1, af[sc][1], acc, 0, 0, 0);
                        float y[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) y[r] = ((acc[r] - mean[sc]) * rstd[sc]) * gv[r] + be[r] + pe[t][r];
                        out[sc][2 * t] = pack_bf16(y[0], y[1]);
                        out[sc][2 * t + 1] = pack_bf16(y[2], y[3]);
                    }
                    __builtin_amdgcn_sched_barrier(0);      // keep the next tile's fragment / parameter reads from piling up (spills)
                }
#pragma unroll
                for (int sc = 0; sc < SB; ++sc)
                    if (s0 + sc < scenes && rows[sc] < g.M) {
                        uint16_t *dst = g.y16 + rows[sc] * N + 64 * G + cofs;
                        // streaming stores: the tokens are consumed by the next kernel from HBM anyway (6.4 GB per 16 scenes), and
                        // dirty lines left in L2 / Infinity Cache were costing that kernel ~4 % while they drained
                        __builtin_nontemporal_store(u32x4{out[sc][0], out[sc][1], out[sc][2], out[sc][3]}, reinterpret_cast<u32x4 *>(dst));
                        __builtin_nontemporal_store(u32x4{out[sc][4], out[sc][5], out[sc][6], out[sc][7]}, reinterpret_cast<u32x4 *>(dst + 8));
                    }
            }
        }
    }
}

template <int NG> int launch_gemm_ln_rows(const GemmLnArgs &g, hipStream_t st) {
    constexpr int SB = 4;
    const size_t lds = (size_t)NG * 64 * 128 + (size_t)3 * NG * 64 * sizeof(float);
    static LvqLdsOnce once;
    if (!lvq_ensure_lds(once, {(const void *)k_gemm_ln_rows<NG, SB>}, lds)) return LVQ_EUNSUPPORTED;
    int scenes = 1;
    int64_t rps = g.M;
    if (g.post && g.M > g.post_rows) { scenes = (int)(g.M / g.post_rows); rps = g.post_rows; }
    const int64_t n_pt = lvq_cdiv(rps, 16);
    const int n_cu = lvq_cu_count();
    const int64_t want = lvq_cdiv(n_pt, LNR_WAVES);
    const unsigned grid = (unsigned)(want < n_cu ? want : n_cu);
    hipLaunchKernelGGL((k_gemm_ln_rows<NG, SB>), dim3(grid), dim3(LNR_WAVES * 64), lds, st, g, (int)n_pt, scenes, rps);
    return lvq_launch_status();
}

template <int NT16> int launch_gemm_ln(const GemmLnArgs &g, hipStream_t st) {
    const size_t lds = (size_t)(NT16 * 16 + 64) * 40 * sizeof(uint16_t);      // >= 4 waves x 16 x 68 floats (17 KB) for every NT16 >= 12
    static LvqLdsOnce once;
    if (lds > 64 * 1024 && !lvq_ensure_lds(once, {(const void *)k_gemm_ln<NT16>}, lds)) return LVQ_EUNSUPPORTED;
    hipLaunchKernelGGL(k_gemm_ln<NT16>, dim3((unsigned)lvq_cdiv(g.M, 64)), dim3(256), lds, st, g);
    return lvq_launch_status();
}

__global__ void __launch_bounds__(256) k_cast_bf16(const float *__restrict__ x, int64_t n, uint16_t *__restrict__ hi,
                                                   uint16_t *__restrict__ lo) {
    int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 3 < n) {
        float4 v = *reinterpret_cast<const float4 *>(x + i);
        ushort4 h = make_ushort4(f32_to_bf16(v.x), f32_to_bf16(v.y), f32_to_bf16(v.z), f32_to_bf16(v.w));
        *reinterpret_cast<ushort4 *>(hi + i) = h;
        if (lo) {
            ushort4 l = make_ushort4(f32_to_bf16(v.x - bf16_to_f32(h.x)), f32_to_bf16(v.y - bf16_to_f32(h.y)),
                                     f32_to_bf16(v.z - bf16_to_f32(h.z)), f32_to_bf16(v.w - bf16_to_f32(h.w)));
            *reinterpret_cast<ushort4 *>(lo + i) = l;
        }
    } else {
        for (; i < n; ++i) {
            uint16_t h = f32_to_bf16(x[i]);
            hi[i] = h;
            if (lo) lo[i] = f32_to_bf16(x[i] - bf16_to_f32(h));
        }
    }
}

__global__ void __launch_bounds__(256) k_bf16_to_f32(const uint16_t *__restrict__ hi, const uint16_t *__restrict__ lo, int64_t n,
                                                     float alpha, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = (bf16_to_f32(hi[i]) + (lo ? bf16_to_f32(lo[i]) : 0.f)) * alpha;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// Skinny-M path (M <= 8: one decode step of the language head): C[m, n] = sum_k A[m, k] W[n, k] is a stream over W
// (HBM-bound: 2 N K bytes for 2 M N K flops), which the 64x64 MFMA tile kernel reads with N/64 workgroups and one row-tile of
// useful work each -- 26 us per projection of the 0.5 B decoder, 2.5 ms per token.  Here a wave owns GEMV_R rows of W, lanes split
// K in 16-byte chunks (coalesced 1 KB per row and step), fp32 FMAs, one shuffle reduction at the end, the epilogue of the tile
// kernels (bias, GELU, alpha, residual, row table; f32 / bf16 / bf16-lo outputs).  bf16x3: a_hi w_hi + a_hi w_lo + a_lo w_hi.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void bf8_to_f32(const uint4 v, float (&f)[8]) {
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
    f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
    f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}
// NORM: A is not read as bf16 but produced on the fly as RMSNorm(xf) * gamma rounded to bf16 (hi[, lo]) -- exactly what lvq_rmsnorm
// writes (same per-lane summation order, same expression), so the result is bit-identical to the rmsnorm + GEMV pair while two of
// the ~12 launches of a decoder layer disappear (a one-row norm kernel costs 12.8 us of dependent latency, 0.63 ms per token).
// QG: the activation is QuickGELU (LVQ_GEMM_QUICK_GELU) and `gelu` is not read; QG = false is the kernel as it always was, with its
// run-time exact-erf switch
template <int MM, bool X3, int GEMV_R, int PRO, bool QG = false>
__global__ void __launch_bounds__(256) k_gemv(const uint16_t *__restrict__ a, const uint16_t *__restrict__ a_lo, const uint16_t *__restrict__ w,
                                              const uint16_t *__restrict__ w_lo, const float *__restrict__ bias, const float *__restrict__ residual,
                                              const float *__restrict__ rowtab, int64_t rowtab_rows, float alpha, int gelu, int m, int n, int k,
                                              int64_t lda, int64_t ldw, int64_t ldc, float *__restrict__ c32, uint16_t *__restrict__ c16,
                                              uint16_t *__restrict__ c16lo, const float *__restrict__ xf, const float *__restrict__ gamma,
                                              float eps) {
    const int lane = threadIdx.x & 63;
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * GEMV_R;
    if (n0 >= n) return;
    constexpr bool NORM = PRO == 1;
    float rstd[MM];
    if (NORM) {
        // lvq_rmsnorm's statistics: lane-strided sum of squares (k = lane, lane + 64, ...), butterfly wave sum, IEEE 1/sqrt
#pragma unroll
        for (int mi = 0; mi < MM; ++mi) {
            float v = 0.f;
            if (mi < m)
                for (int kk = lane; kk < k; kk += 64) {
                    const float t = xf[(int64_t)mi * k + kk];
                    v += t * t;
                }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            rstd[mi] = 1.0f / sqrtf(v / (float)k + eps);
        }
    }
    float acc[MM][GEMV_R];
#pragma unroll
    for (int mi = 0; mi < MM; ++mi)
#pragma unroll
        for (int r = 0; r < GEMV_R; ++r) acc[mi][r] = 0.f;
    for (int k0 = lane * 8; k0 < k; k0 += 64 * 8) {
        float af[MM][8], al[X3 ? MM : 1][8];
#pragma unroll
        for (int mi = 0; mi < MM; ++mi) {
            const bool live = mi < m;
            if (NORM) {
                const float4 x0 = live ? *reinterpret_cast<const float4 *>(xf + (int64_t)mi * k + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 x1 = live ? *reinterpret_cast<const float4 *>(xf + (int64_t)mi * k + k0 + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 g0 = *reinterpret_cast<const float4 *>(gamma + k0), g1 = *reinterpret_cast<const float4 *>(gamma + k0 + 4);
                const float xs[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
                const float gs[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float y = gs[j] * ((xs[j] - 0.f) * rstd[mi]);          // k_norm<true>: gamma[k] * ((x - mean) * rstd), mean = 0
                    const uint16_t h = f32_to_bf16(y);
                    af[mi][j] = bf16_to_f32(h);
                    if (X3) al[mi][j] = bf16_to_f32(f32_to_bf16(y - bf16_to_f32(h)));
                }
            } else {
                bf8_to_f32(live ? *reinterpret_cast<const uint4 *>(a + mi * lda + k0) : make_uint4(0u, 0u, 0u, 0u), af[mi]);
                if (X3) bf8_to_f32(live ? *reinterpret_cast<const uint4 *>(a_lo + mi * lda + k0) : make_uint4(0u, 0u, 0u, 0u), al[mi]);
            }
        }
#pragma unroll
        for (int r = 0; r < GEMV_R; ++r) {
            const int nr = n0 + r < n ? n0 + r : n - 1;            // clamp: the tail rows are computed twice, stored once
            float wf[8], wl[8];
            bf8_to_f32(*reinterpret_cast<const uint4 *>(w + (int64_t)nr * ldw + k0), wf);
            if (X3) bf8_to_f32(*reinterpret_cast<const uint4 *>(w_lo + (int64_t)nr * ldw + k0), wl);
#pragma unroll
            for (int mi = 0; mi < MM; ++mi)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    acc[mi][r] = fmaf(af[mi][j], wf[j], acc[mi][r]);
                    if (X3) {
                        acc[mi][r] = fmaf(af[mi][j], wl[j], acc[mi][r]);
                        acc[mi][r] = fmaf(al[mi][j], wf[j], acc[mi][r]);
                    }
                }
        }
    }
#pragma unroll
    for (int mi = 0; mi < MM; ++mi)
#pragma unroll
        for (int r = 0; r < GEMV_R; ++r) {
            float v = acc[mi][r];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
            acc[mi][r] = v;
        }
    if (lane < MM * GEMV_R) {
        const int mi = lane / GEMV_R, r = lane % GEMV_R, col = n0 + r;
        if (mi < m && col < n) {
            float x = 0.f;
#pragma unroll
            for (int a_ = 0; a_ < MM; ++a_)
#pragma unroll
                for (int b_ = 0; b_ < GEMV_R; ++b_)
                    if (a_ == mi && b_ == r) x = acc[a_][b_];
            if (bias) x += bias[col];
            if (QG) x = gelu_quick(x);
            else if (gelu) x = gelu_erf(x);
            x *= alpha;
            const int64_t o = (int64_t)mi * ldc + col;
            if (residual) x += residual[o];
            if (rowtab) x += rowtab[(int64_t)(mi % rowtab_rows) * n + col];
            if (c32) c32[o] = x;
            if (c16) {
                const uint16_t h = f32_to_bf16(x);
                c16[o] = h;
                if (c16lo) c16lo[o] = f32_to_bf16(x - bf16_to_f32(h));
            }
        }
    }
}


// gelu: 0 none, 1 exact erf, 2 QuickGELU (k_gemv<.., QG = true>; the RMSNorm prologue form has no caller that asks for it)
template <int MM, int R, int PRO>
static void launch_gemv_r(bool x3, hipStream_t st, const uint16_t *a, const uint16_t *a_lo, const uint16_t *w, const uint16_t *w_lo,
                          const float *bias, const float *residual, const float *rowtab, int64_t rowtab_rows, float alpha, int gelu, int m, int n,
                          int k, int64_t lda, int64_t ldw, int64_t ldc, float *c32, uint16_t *c16, uint16_t *c16lo, const float *xf,
                          const float *gamma, float eps) {
    const dim3 grid((unsigned)lvq_cdiv(n, 4 * R));
    if constexpr (PRO == 0) {
        if (gelu == 2) {
            if (x3) hipLaunchKernelGGL((k_gemv<MM, true, R, 0, true>), grid, dim3(256), 0, st, a, a_lo, w, w_lo, bias, residual, rowtab, rowtab_rows, alpha,
                                       gelu, m, n, k, lda, ldw, ldc, c32, c16, c16lo, xf, gamma, eps);
            else hipLaunchKernelGGL((k_gemv<MM, false, R, 0, true>), grid, dim3(256), 0, st, a, a_lo, w, w_lo, bias, residual, rowtab, rowtab_rows, alpha,
                                    gelu, m, n, k, lda, ldw, ldc, c32, c16, c16lo, xf, gamma, eps);
            return;
        }
    }
    if (x3) hipLaunchKernelGGL((k_gemv<MM, true, R, PRO>), grid, dim3(256), 0, st, a, a_lo, w, w_lo, bias, residual, rowtab, rowtab_rows, alpha, gelu, m,
                               n, k, lda, ldw, ldc, c32, c16, c16lo, xf, gamma, eps);
    else hipLaunchKernelGGL((k_gemv<MM, false, R, PRO>), grid, dim3(256), 0, st, a, a_lo, w, w_lo, bias, residual, rowtab, rowtab_rows, alpha, gelu, m,
                            n, k, lda, ldw, ldc, c32, c16, c16lo, xf, gamma, eps);
}
// rows of W per wave: 4 when N alone fills the chip (A reuse), 1 for narrow outputs (896-wide o_proj / down_proj: 224 waves of
// 4 rows left 3/4 of the SIMDs idle, 9.2 us; one row per wave spreads the same stream over 896 waves)
template <int PRO>
static void launch_gemv(bool x3, hipStream_t st, const uint16_t *a, const uint16_t *a_lo, const uint16_t *w, const uint16_t *w_lo,
                        const float *bias, const float *residual, const float *rowtab, int64_t rowtab_rows, float alpha, int gelu, int m, int n,
                        int k, int64_t lda, int64_t ldw, int64_t ldc, float *c32, uint16_t *c16, uint16_t *c16lo, const float *xf,
                        const float *gamma, float eps) {
#define LVQ_GV(MM, R) launch_gemv_r<MM, R, PRO>(x3, st, a, a_lo, w, w_lo, bias, residual, rowtab, rowtab_rows, alpha, gelu, m, n, k, lda, ldw, ldc, c32, c16, c16lo, xf, gamma, eps)
    const bool wide = n >= 4096;
    if (m <= 1) { if (wide) LVQ_GV(1, 4); else LVQ_GV(1, 1); }
    else if (m <= 2) { if (wide) LVQ_GV(2, 4); else LVQ_GV(2, 1); }
    else if (m <= 4) { if (wide) LVQ_GV(4, 4); else LVQ_GV(4, 1); }
    else { if (wide) LVQ_GV(8, 4); else LVQ_GV(8, 1); }
#undef LVQ_GV
}

// RMSNorm fused into the skinny-M projection (decode step): C = epi(RMSNorm(x) * gamma @ W^T), x [m, k] fp32, m <= 8.
extern "C" int lvq_gemv_rmsnorm_bf16(const float *x, const float *gamma, float eps, const lvq_bf16 *w, const lvq_bf16 *w_lo, const float *bias,
                                     int m, int n, int k, int64_t ldw, int64_t ldc, float *c_f32, lvq_bf16 *c_bf16, lvq_bf16 *c_lo,
                                     lvq_stream_t stream) {
    if (m <= 0 || m > 8 || n <= 0 || k <= 0 || !x || !gamma || !w || (!c_f32 && !c_bf16) || (c_lo && !c_bf16)) return LVQ_EINVAL;
    if ((k & 7) || (ldw & 7) || ldw < k || ldc < n) return LVQ_EUNSUPPORTED;
    if (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)w | (uintptr_t)w_lo) & 15) return LVQ_EUNSUPPORTED;
    launch_gemv<1>(w_lo != nullptr, lvq_s(stream), nullptr, nullptr, w, w_lo, bias, nullptr, nullptr, 1, 1.0f, 0, m, n, k, k, ldw, ldc, c_f32, c_bf16,
                      c_lo, x, gamma, eps);
    return lvq_launch_status();
}

extern "C" int lvq_gemm_bf16(const lvq_bf16 *a, const lvq_bf16 *a_lo, const lvq_bf16 *w, const lvq_bf16 *w_lo,
                             const float *bias, const float *residual, const float *rowtab, int64_t rowtab_rows,
                             float alpha, int flags, int64_t m, int n, int k, int64_t lda, int64_t ldw, int64_t ldc,
                             int batch, int64_t a_bs, int64_t w_bs, int64_t c_bs, float *c_f32, lvq_bf16 *c_bf16,
                             lvq_bf16 *c_lo, lvq_stream_t stream) {
    if (m < 0 || n <= 0 || k <= 0 || batch <= 0 || !a || !w || (!c_f32 && !c_bf16)) return LVQ_EINVAL;
    // operand forms: plain (no lo parts), bf16x3 (a and w as hi + lo: hi*hi + hi*lo + lo*hi), and "x2w" (a plain, w hi + lo:
    // a*w_hi + a*w_lo) -- the K|V projection of the "mixed" mode, where the per-row rounding of A averages out over the key
    // stream but the rounding of W is common to every key
    if (a_lo != nullptr && w_lo == nullptr) return LVQ_EINVAL;
    if (c_lo && !c_bf16) return LVQ_EINVAL;
    if (rowtab && rowtab_rows <= 0) return LVQ_EINVAL;
    if ((flags & LVQ_GEMM_GELU) && (flags & LVQ_GEMM_QUICK_GELU)) return LVQ_EINVAL;      // one activation per call
    if (m == 0) return LVQ_OK;
    // activation of the epilogue = the kernels' GELU template value: 0 none, 1 exact erf, 2 QuickGELU
    const int act = (flags & LVQ_GEMM_QUICK_GELU) ? 2 : (flags & LVQ_GEMM_GELU) ? 1 : 0;
    // 16-byte operand loads: K, leading dims and batch strides in multiples of 8 elements, 16-B aligned bases
    if ((k & 7) || (lda & 7) || (ldw & 7) || (a_bs & 7) || (w_bs & 7) || lda < k || ldw < k || ldc < n)
        return LVQ_EUNSUPPORTED;
    if (((uintptr_t)a | (uintptr_t)w | (uintptr_t)a_lo | (uintptr_t)w_lo) & 15) return LVQ_EUNSUPPORTED;
    if (m <= 8 && batch == 1 && n >= 64 && (a_lo != nullptr || w_lo == nullptr) && !lvq_tune().gemm_no_gemv) {   // skinny M: stream W once (k_gemv)
        launch_gemv<0>(a_lo != nullptr, lvq_s(stream), a, a_lo, w, w_lo, bias, residual, rowtab, rowtab_rows, alpha, act,
                           (int)m, n, k, lda, ldw, ldc, c_f32, c_bf16, c_lo, nullptr, nullptr, 0.f);
        return lvq_launch_status();
    }
    GemmArgs g;
    g.m_dev = nullptr;
    g.nseg = a_lo ? 3 : (w_lo ? 2 : 1);
    g.a[0] = a; g.w[0] = w;
    g.a[1] = a; g.w[1] = w_lo;
    g.a[2] = a_lo; g.w[2] = w;
    g.bias = bias; g.residual = residual; g.rowtab = rowtab; g.rowtab_rows = rowtab_rows;
    g.alpha = alpha; g.flags = flags; g.M = m; g.N = n; g.K = k;
    g.lda = lda; g.ldw = ldw; g.ldc = ldc; g.a_bs = a_bs; g.w_bs = w_bs; g.c_bs = c_bs;
    g.c32 = c_f32; g.c16 = c_bf16; g.c16lo = c_lo;
    // C (and the residual read) streams past the caches when >= 32 MB are written: non-temporal stores / loads.  Measured on the
    // headline cross-attention (32768 x 196): 0.256 -> 0.238 ms -- streaming even its 50 MB Q projection beats leaving it in
    // the Infinity Cache; neutral on the full pipeline, whose big projections stream already.
    {
        const int64_t c_bytes = (int64_t)m * n * batch * ((c_f32 ? 4 : 0) + (c_bf16 ? 2 : 0) + (c_lo ? 2 : 0));
        const int mb = lvq_tune().gemm_stream_c_mb;
        const int64_t thr = (int64_t)(mb > 0 ? mb : 32) << 20;
        g.stream_c = c_bytes >= thr && mb >= 0;
    }
    g.vec_epilogue = (n % 8 == 0) && (ldc % 8 == 0) && (c_bs % 8 == 0) &&
                     !(((uintptr_t)c_f32 | (uintptr_t)residual | (uintptr_t)bias | (uintptr_t)rowtab) & 15) &&
                     !(((uintptr_t)c_bf16 | (uintptr_t)c_lo) & 15);
    hipStream_t st = lvq_s(stream);
    const int64_t big_tiles = lvq_cdiv(m, 128) * lvq_cdiv(n, 128) * batch;
    const bool dma = (k % 64) == 0;      // LDS-DMA path needs whole 64-wide K tiles (no per-chunk zero fill)
    // 256x128 / 8 waves / 3 stages when there is enough work to fill the chip with the bigger tile
    const bool huge = dma && lvq_cdiv(m, 256) * lvq_cdiv(n, 128) * batch >= 512 && !lvq_tune().gemm_no256;
    if (batch > 65535) return LVQ_EUNSUPPORTED;
    // 256x256 / two 64-KiB slots: 2/3 of the L2->LDS fill bytes of the 256x128 tile (the bound on these projections);
    // whole tiles only, and enough of them that the coarser grid still fills the 256 CUs several times over
    static LvqLdsOnce once256;      // per device: did the runtime grant 160 KiB of dynamic LDS?
    // ... or, below that, when one tile per CU keeps >= 80 % of the CUs of its last dispatch round busy (18432 x 768: 216 tiles in one
    // round, 0.150 -> ~0.1 ms per x3 GEMM of the query side; 260 tiles would be two rounds for four tiles and stay on the smaller kernels)
    const int64_t min256 = lvq_tune().gemm_256x256_min_tiles > 0 ? lvq_tune().gemm_256x256_min_tiles : 1024;
    const int64_t t256 = (m / 256) * (n / 256) * batch, cus = lvq_cu_count();
    const bool round_ok = t256 >= 200 && t256 * 5 >= ((t256 + cus - 1) / cus) * cus * 4;
    if (dma && g.vec_epilogue && m % 256 == 0 && n % 256 == 0 && (t256 >= min256 || (round_ok && lvq_tune().gemm_256x256_min_tiles <= 0)) &&
        (m / 256) * (n / 256) <= 0x7fffffff && !lvq_tune().gemm_no256x256 && !lvq_tune().gemm_no256) {
        const size_t lds = (size_t)5 * 256 * 128;              // A ring 3 x 32 KiB + W ring 2 x 32 KiB
        if (lvq_ensure_lds(once256, {(const void *)k_gemm_256<0, 0>, (const void *)k_gemm_256<1, 0>, (const void *)k_gemm_256<0, 1>,
                                     (const void *)k_gemm_256<1, 1>, (const void *)k_gemm_256<2, 0>, (const void *)k_gemm_256<2, 1>}, lds)) {
            g.ntx = (int)(n / 256);
            dim3 grid((unsigned)((m / 256) * (n / 256)), 1, (unsigned)batch);
            const bool ant = g.ntx <= 8;
            if (act == 2)      { if (ant) hipLaunchKernelGGL((k_gemm_256<2, 1>), grid, dim3(512), lds, st, g); else hipLaunchKernelGGL((k_gemm_256<2, 0>), grid, dim3(512), lds, st, g); }
            else if (act == 1) { if (ant) hipLaunchKernelGGL((k_gemm_256<1, 1>), grid, dim3(512), lds, st, g); else hipLaunchKernelGGL((k_gemm_256<1, 0>), grid, dim3(512), lds, st, g); }
            else    { if (ant) hipLaunchKernelGGL((k_gemm_256<0, 1>), grid, dim3(512), lds, st, g); else hipLaunchKernelGGL((k_gemm_256<0, 0>), grid, dim3(512), lds, st, g); }
            return lvq_launch_status();
        }
    }
    if (huge) {
        const int64_t tiles = lvq_cdiv(n, 128) * lvq_cdiv(m, 256);
        if (tiles > 0x7fffffff) return LVQ_EUNSUPPORTED;
        g.ntx = (int)lvq_cdiv(n, 128);
        const size_t lds = (size_t)3 * (256 + 128) * 128;
        static LvqLdsOnce once;
        if (!lvq_ensure_lds(once, {(const void *)k_gemm_bf16<256, 128, 1, 0, 8>, (const void *)k_gemm_bf16<256, 128, 1, 1, 8>,
                                   (const void *)k_gemm_bf16<256, 128, 1, 2, 8>}, lds)) return LVQ_ELAUNCH;
        dim3 grid((unsigned)tiles, 1, (unsigned)batch);
        if (act == 2)      hipLaunchKernelGGL((k_gemm_bf16<256, 128, 1, 2, 8>), grid, dim3(512), lds, st, g);
        else if (act == 1) hipLaunchKernelGGL((k_gemm_bf16<256, 128, 1, 1, 8>), grid, dim3(512), lds, st, g);
        else    hipLaunchKernelGGL((k_gemm_bf16<256, 128, 1, 0, 8>), grid, dim3(512), lds, st, g);
        return lvq_launch_status();
    }
    const int bm = big_tiles >= 192 ? 128 : 64;
    const int64_t tiles = lvq_cdiv(n, bm) * lvq_cdiv(m, bm);
    if (tiles > 0x7fffffff) return LVQ_EUNSUPPORTED;
    g.ntx = (int)lvq_cdiv(n, bm);
    dim3 grid((unsigned)tiles, 1, (unsigned)batch);
    const size_t lds = (size_t)((bm == 64 && dma) ? 3 : 2) * (bm + bm) * 128;
#define LVQ_LAUNCH(BM_, DMA_, GE_) hipLaunchKernelGGL((k_gemm_bf16<BM_, BM_, DMA_, GE_, 4>), grid, dim3(256), lds, st, g)
#define LVQ_LAUNCH_ACT(BM_, DMA_) do { if (act == 2) LVQ_LAUNCH(BM_, DMA_, 2); else if (act == 1) LVQ_LAUNCH(BM_, DMA_, 1); else LVQ_LAUNCH(BM_, DMA_, 0); } while (0)
    if (bm == 128) {
        if (dma) LVQ_LAUNCH_ACT(128, 1); else LVQ_LAUNCH_ACT(128, 0);
    } else {
        if (dma) LVQ_LAUNCH_ACT(64, 1); else LVQ_LAUNCH_ACT(64, 0);
    }
#undef LVQ_LAUNCH_ACT
#undef LVQ_LAUNCH
    return lvq_launch_status();
}

// The K|V projection over the LIVE rows of the sparse BEV stream (bev_tiles.hip): c[0 .. *m_rows_dev) = a @ w^T + bias on the 256 x 256
// tile kernel, rows past the device-side count untouched.  m_cap (the buffers' row capacity) and n multiples of 256, k of 64.
extern "C" int lvq_gemm_bf16_live_rows(const lvq_bf16 *a, const lvq_bf16 *a_lo, const lvq_bf16 *w, const lvq_bf16 *w_lo, const float *bias,
                                       int64_t m_cap, const int32_t *m_rows_dev, int n, int k, int64_t lda, int64_t ldw, int64_t ldc,
                                       lvq_bf16 *c_bf16, lvq_bf16 *c_lo, lvq_stream_t stream) {
    if (m_cap <= 0 || n <= 0 || k <= 0 || !a || !w || !c_bf16 || !m_rows_dev) return LVQ_EINVAL;
    if (a_lo != nullptr && w_lo == nullptr) return LVQ_EINVAL;
    if ((m_cap % 256) || (n % 256) || (k % 64) || (lda & 7) || (ldw & 7) || (ldc & 7) || lda < k || ldw < k || ldc < n) return LVQ_EUNSUPPORTED;
    if (((uintptr_t)a | (uintptr_t)w | (uintptr_t)a_lo | (uintptr_t)w_lo | (uintptr_t)c_bf16 | (uintptr_t)c_lo | (uintptr_t)bias) & 15) return LVQ_EUNSUPPORTED;
    if ((m_cap / 256) * (n / 256) > 0x7fffffff) return LVQ_EUNSUPPORTED;
    GemmArgs g;
    g.m_dev = m_rows_dev;
    g.nseg = a_lo ? 3 : (w_lo ? 2 : 1);
    g.a[0] = a; g.w[0] = w; g.a[1] = a; g.w[1] = w_lo; g.a[2] = a_lo; g.w[2] = w;
    g.bias = bias; g.residual = nullptr; g.rowtab = nullptr; g.rowtab_rows = 0; g.alpha = 1.0f; g.flags = 0;
    g.M = m_cap; g.N = n; g.K = k; g.lda = lda; g.ldw = ldw; g.ldc = ldc; g.a_bs = 0; g.w_bs = 0; g.c_bs = 0;
    g.c32 = nullptr; g.c16 = c_bf16; g.c16lo = c_lo; g.stream_c = 1; g.vec_epilogue = 1;
    g.ntx = n / 256;
    const size_t lds = (size_t)5 * 256 * 128;
    static LvqLdsOnce once;
    if (!lvq_ensure_lds(once, {(const void *)k_gemm_256<0, 0>, (const void *)k_gemm_256<0, 1>}, lds)) return LVQ_ELAUNCH;
    dim3 grid((unsigned)((m_cap / 256) * (n / 256)), 1, 1);
    if (g.ntx <= 8) hipLaunchKernelGGL((k_gemm_256<0, 1>), grid, dim3(512), lds, lvq_s(stream), g);
    else            hipLaunchKernelGGL((k_gemm_256<0, 0>), grid, dim3(512), lds, lvq_s(stream), g);
    return lvq_launch_status();
}

extern "C" int lvq_cast_bf16(const float *x, int64_t n, lvq_bf16 *hi, lvq_bf16 *lo, lvq_stream_t stream) {
    if (n < 0 || (n > 0 && (!x || !hi))) return LVQ_EINVAL;
    if (n == 0) return LVQ_OK;
    if (((uintptr_t)x & 15) || ((uintptr_t)hi & 7) || ((uintptr_t)lo & 7)) return LVQ_EUNSUPPORTED;
    hipLaunchKernelGGL(k_cast_bf16, dim3((unsigned)lvq_cdiv(n, 1024)), dim3(256), 0, lvq_s(stream), x, n, hi, lo);
    return lvq_launch_status();
}

extern "C" int lvq_bf16_to_f32(const lvq_bf16 *hi, const lvq_bf16 *lo, int64_t n, float alpha, float *out, lvq_stream_t stream) {
    if (n < 0 || (n > 0 && (!hi || !out))) return LVQ_EINVAL;
    if (n == 0) return LVQ_OK;
    hipLaunchKernelGGL(k_bf16_to_f32, dim3((unsigned)lvq_cdiv(n, 256)), dim3(256), 0, lvq_s(stream), hi, lo, n, alpha, out);
    return lvq_launch_status();
}

extern "C" int lvq_gemm_ln_bf16(const lvq_bf16 *a, const lvq_bf16 *a_lo, const lvq_bf16 *w, const lvq_bf16 *w_lo, const float *bias,
                                const float *gamma, const float *beta, float eps, const float *post_add, int64_t post_rows,
                                int64_t m, int n, int k, int64_t lda, int64_t ldw, lvq_bf16 *y_bf16, lvq_bf16 *y_lo,
                                lvq_stream_t stream) {
    if (m < 0 || n <= 0 || k <= 0 || !a || !w || !gamma || !y_bf16) return LVQ_EINVAL;
    if ((a_lo == nullptr) != (w_lo == nullptr)) return LVQ_EINVAL;
    if (post_add && post_rows <= 0) return LVQ_EINVAL;
    if (m == 0) return LVQ_OK;
    if ((k & 31) || k > 256 || (lda & 7) || (ldw & 7) || lda < k || ldw < k) return LVQ_EUNSUPPORTED;
    if (((uintptr_t)a | (uintptr_t)w | (uintptr_t)a_lo | (uintptr_t)w_lo | (uintptr_t)bias | (uintptr_t)gamma | (uintptr_t)beta |
         (uintptr_t)post_add | (uintptr_t)y_bf16 | (uintptr_t)y_lo) & 15)
        return LVQ_EUNSUPPORTED;
    if (lvq_cdiv(m, 64) > 0x7fffffff) return LVQ_EUNSUPPORTED;
    GemmLnArgs g;
    g.nseg = a_lo ? 3 : (w_lo ? 2 : 1);
    g.a[0] = a; g.w[0] = w; g.a[1] = a; g.w[1] = w_lo; g.a[2] = a_lo; g.w[2] = w;
    g.bias = bias; g.gamma = gamma; g.beta = beta; g.post = post_add; g.post_rows = post_rows; g.eps = eps;
    g.M = m; g.N = n; g.K = k; g.lda = lda; g.ldw = ldw; g.y16 = y_bf16; g.y16lo = y_lo;
    g.scenes = 0;
    if (post_add && post_rows % 512 == 0 && m % post_rows == 0 && m / post_rows > 1 && m / post_rows <= 4096)
        g.scenes = (int)(m / post_rows);            // whole tiles per scene, tiles-per-scene a multiple of the 8 XCDs
    hipStream_t st = lvq_s(stream);
    // K = 64, plain bf16, table rows aligned to scenes: the row-streaming kernel (W resident in LDS, table read once)
    if (g.nseg == 1 && k == 64 && n % 64 == 0 && n <= 1024 && lvq_cdiv(m, 16) <= 0x7fffffff && !lvq_tune().gemm_ln_tiles &&
        (!post_add || m <= post_rows || (post_rows % 16 == 0 && m % post_rows == 0))) {
        int rc = LVQ_EUNSUPPORTED;
        switch (n) {
            case 256: rc = launch_gemm_ln_rows<4>(g, st); break;
            case 512: rc = launch_gemm_ln_rows<8>(g, st); break;
            case 768: rc = launch_gemm_ln_rows<12>(g, st); break;
            case 896: rc = launch_gemm_ln_rows<14>(g, st); break;
            case 1024: rc = launch_gemm_ln_rows<16>(g, st); break;
            default: break;
        }
        if (rc != LVQ_EUNSUPPORTED) return rc;
    }
    switch (n) {   // row-complete tiles: one instantiation per supported d_model
        case 256: return launch_gemm_ln<16>(g, st);
        case 512: return launch_gemm_ln<32>(g, st);
        case 768: return launch_gemm_ln<48>(g, st);
        case 896: return launch_gemm_ln<56>(g, st);
        case 1024: return launch_gemm_ln<64>(g, st);
        default: return LVQ_EUNSUPPORTED;
    }
}
