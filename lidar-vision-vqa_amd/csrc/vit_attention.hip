// csrc/vit_attention.hip -- self-attention over a 2-D token grid with the decomposed relative-position bias of the SAM / ViTDet
// image encoder formed INSIDE the kernel (deepencoder/sam_vary_sdpa.py:269-296, 348-413):
//
//   O[b, i, h, :] = softmax_j( scale q_i.k_j + q_i.Rh[y_i - y_j + gh - 1] + q_i.Rw[x_i - x_j + gw - 1] ) v_j
//
// i = y_i gw + x_i and j = y_j gw + x_j index the gh x gw grid of batch entry b (a window, or a whole image).  The reference
// materialises the bias as a dense [B, H, N, N] fp32 array (805 MB for one global block of SAM-B); here nothing of size N x N
// exists anywhere: a workgroup needs the two tables [2gh-1, 64] and [2gw-1, 64] and its own queries.
//
// Structure: attention.hip's fused flash kernel (k_attn, DHP = 64, 4 waves x 16 queries, S^T = K Q^T so the query sits on
// lane & 15 and the softmax statistics are register reductions) with one extra prologue per wave:
//   T^T = [Rh; Rw] Q^T        one MFMA product, <= 254 table rows x 16 queries, 64 deep, hi + lo like the scores in bf16x3
// whose C layout (query on lane & 15, four table rows in the lane's registers) is written to LDS as fp32 T[query][row].  In the
// key loop a score then takes two shifted LDS reads of its own query's row: T[q][gh - 1 + y_i - y_j] and
// T[q][2gh - 1 + gw - 1 + x_i - x_j]; the lane's base addresses carry (y_i, x_i), the key's (y_j, x_j) come from one
// multiply by 1 / gw per key (exact for j < 4096).  The bias uses the UNSCALED q (as the reference does), so Q is not pre-scaled
// in either precision mode: scores and bias meet in the log2 domain in one fma.
//
// A wave keeps only the window of each table that its 16 queries read (rel_tab_stride below): 143 rows instead of 254 on the
// 64 x 64 grid.  LDS: T 4 waves x 16 queries x stride fp32 (11 KB at 14 x 14, 36 KB at 64 x 64) + one or two K|V stages of 64
// keys (18 KB each plain, 36 KB bf16x3) -- 72 KB at 64 x 64 in either form (two workgroups per CU), 120 KB at worst, sized per launch.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

struct RelArgs {
    const uint16_t *qkv, *qkvl;       // packed [B * gh * gw, >= 3 H 64]: column = part * H * 64 + h * 64 + e
    const uint16_t *rh, *rhl, *rw, *rwl;
    int B, H, gh, gw, nqt;
    int ts;                           // fp32 elements per query row of the bias table in LDS (rel_tab_stride)
    int64_t ld, ldo;
    float scale;
    uint16_t *o, *ol;
};

constexpr int KVB = 64;           // keys per tile
constexpr int DH = 64;
constexpr int KROW = DH + 8;      // padded K / V row in LDS (bf16 elements)
constexpr int NW = 4;
constexpr int NT = NW * 64;
constexpr int CH = DH / 8;
constexpr int NLD = KVB * CH / NT;     // 16-byte chunks per thread per operand part: 2
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
    bf16x2_t p = {(__bf16)a, (__bf16)b};
    return *reinterpret_cast<uint32_t *>(&p);
}
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float max_over_groups(float x) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

// Table rows a wave needs.  Its 16 consecutive queries span rows y_min .. y_max of the grid, and query (y, x) reads T_h rows
// [y, y + gh) and T_w rows [x, x + gw): the wave's window of Rh is [y_min, y_max + gh), of Rw [x_min, x_max + gw) when the queries
// share one row and all of it otherwise.  A wave starts at a multiple of 16, so it stays in one row whenever gw % 16 == 0 (then
// x_max - x_min <= 15), and spans at most ceil(15 / gw) row steps otherwise.  The bound sizes the LDS rows; the kernel's own
// window never exceeds it.
static inline int rel_tab_stride(int gh, int gw) {
    const bool one_row = gw % 16 == 0;
    int span = one_row ? 0 : (15 + gw - 1) / gw;
    if (span > gh - 1) span = gh - 1;
    const int nh = gh + span, nw = one_row ? gw + 15 : 2 * gw - 1;
    return (nh + nw) | 1;                                                   // odd: the 16 queries of a wave land on different banks
}
static inline size_t rel_lds_bytes(int gh, int gw, bool split, int stages) {
    return (size_t)NW * 16 * rel_tab_stride(gh, gw) * 4 + (size_t)stages * 2 * (split ? 2 : 1) * KVB * KROW * 2;
}
constexpr size_t LDS_CU = 160 * 1024;
static inline size_t rel_lds_max() {
    size_t m = 0;
    for (int gh = 1; gh <= 64; ++gh)
        for (int gw = 1; gw <= 64; ++gw) m = rel_lds_bytes(gh, gw, true, 2) > m ? rel_lds_bytes(gh, gw, true, 2) : m;
    return m;
}
// K | V stages: two (the next tile is written while this one is read: one barrier per tile) unless one stage lets more workgroups share
// a CU -- the 64 x 64 grid in the hi + lo form runs two workgroups per CU with one stage and a single one with two
static inline int rel_stages(int gh, int gw, bool split) {
    return LDS_CU / rel_lds_bytes(gh, gw, split, 1) > LDS_CU / rel_lds_bytes(gh, gw, split, 2) ? 1 : 2;
}

template <int NSPLIT, int STAGES>
__global__ void __launch_bounds__(NT) k_attn_relpos(RelArgs a) {
    constexpr int NS = (NSPLIT == 3) ? 2 : 1;
    constexpr int NC = DH / 32, ND = DH / 16;
    constexpr int TILE_E = 2 * NS * KVB * KROW;
    extern __shared__ __attribute__((aligned(16))) uint16_t smem[];
    // [STAGES][Ks [NS][64][KROW] | Vs [NS][64][KROW]] | T [NW][16][TS] fp32
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, l15 = lane & 15;
    const int N = a.gh * a.gw, d = a.H * DH;
    const int TS = a.ts;
    const int grp = blockIdx.x / a.nqt, qtile = blockIdx.x - grp * a.nqt;
    const int h = grp % a.H, b = grp / a.H;
    const int q0 = qtile * (NW * 16) + wid * 16;
    const int qi = q0 + l15;
    const float cexp = a.scale * LOG2E;

    // Q fragments (B operand): lane supplies Q[qi][c * 32 + 8 g .. + 7], unscaled
    bf16x8 qf[NS][NC];
    {
        const uint16_t *src[2] = {a.qkv, a.qkvl};
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                uint4 v = make_uint4(0, 0, 0, 0);
                if (qi < N) v = *reinterpret_cast<const uint4 *>(src[s] + ((int64_t)b * N + qi) * a.ld + (int64_t)h * DH + c * 32 + g * 8);
                qf[s][c] = *reinterpret_cast<bf16x8 *>(&v);
            }
    }

    // ---- T^T = [Rh; Rw] Q^T for this wave's 16 queries -> LDS (fp32), restricted to the table rows the wave reads (see
    // rel_tab_stride): local row r is Rh row lo_h + r for r < nh, Rw row lo_w + r - nh above.  A operand straight from global: lane
    // supplies local row blk * 16 + l15, columns c * 32 + 8 g .. + 7; C: lane (query l15, group g) holds local rows blk * 16 + 4 g + r ----
    const float rgw = 1.0f / (float)a.gw;
    auto coords = [&](int j, int &y, int &x) { y = (int)(((float)j + 0.5f) * rgw); x = j - y * a.gw; };       // exact for j < 4096
    int y0, x0, y1, x1, yi, xi;
    coords(q0 < N ? q0 : N - 1, y0, x0);
    coords(q0 + 15 < N ? q0 + 15 : N - 1, y1, x1);
    coords(qi < N ? qi : N - 1, yi, xi);                               // a query past N reads as the last one
    const int lo_h = y0, nh = y1 - y0 + a.gh;
    const int lo_w = y1 == y0 ? x0 : 0, nw = y1 == y0 ? x1 - x0 + a.gw : 2 * a.gw - 1;
    const int ntab = nh + nw;                                          // <= TS by construction
    float *T = reinterpret_cast<float *>(smem + STAGES * TILE_E) + (wid * 16 + l15) * TS;
    for (int blk = 0; blk * 16 < ntab; ++blk) {
        const int row = blk * 16 + l15;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            uint4 th = make_uint4(0, 0, 0, 0), tl = make_uint4(0, 0, 0, 0);
            if (row < ntab) {
                const int64_t off = (int64_t)(row < nh ? lo_h + row : lo_w + row - nh) * DH + c * 32 + g * 8;
                th = *reinterpret_cast<const uint4 *>((row < nh ? a.rh : a.rw) + off);
                if (NSPLIT == 3) tl = *reinterpret_cast<const uint4 *>((row < nh ? a.rhl : a.rwl) + off);
            }
            const bf16x8 rh = *reinterpret_cast<bf16x8 *>(&th), rl = *reinterpret_cast<bf16x8 *>(&tl);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rh, qf[0][c], acc, 0, 0, 0);
            if (NSPLIT == 3) {
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rh, qf[NS - 1][c], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(rl, qf[0][c], acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int tr = blk * 16 + 4 * g + r;
            if (tr < ntab) T[tr] = acc[r] * LOG2E;                 // the bias enters the exponent in the log2 domain
        }
    }
    // the lane's two row bases: Rh row gh - 1 + y_i - ky is local row (gh - 1 + y_i - lo_h) - ky, Rw row gw - 1 + x_i - kx local
    // row nh + (gw - 1 + x_i - lo_w) - kx
    const float *Th = T + a.gh - 1 + yi - lo_h, *Tw = T + nh + a.gw - 1 + xi - lo_w;

    f32x4 o[ND + 1];
#pragma unroll
    for (int n = 0; n <= ND; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY;
    bf16x8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (short)0x3F80;

    const int n_tiles = (N + KVB - 1) / KVB;

    // ---- K / V staging: buffer descriptors cover exactly the valid rows of this (batch, head): rows past N read as zero ----
    const int wave_b = __builtin_amdgcn_readfirstlane(b), wave_h = __builtin_amdgcn_readfirstlane(h);
    __amdgpu_buffer_rsrc_t rk[NS], rv[NS];
    {
        const uint16_t *base[2] = {a.qkv, a.qkvl};
        const uint32_t bytes = (uint32_t)(((int64_t)(N - 1) * a.ld + DH) * 2);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const uint16_t *p = base[s] + (int64_t)wave_b * N * a.ld + (int64_t)wave_h * DH;
            rk[s] = __builtin_amdgcn_make_buffer_rsrc((void *)(p + d), 0, bytes, 0x00020000);
            rv[s] = __builtin_amdgcn_make_buffer_rsrc((void *)(p + 2 * d), 0, bytes, 0x00020000);
        }
    }
    uint32_t goff[NLD], lso[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = tid + NT * i, r = e / CH, kk = (e - r * CH) * 8;
        goff[i] = (uint32_t)((r * a.ld + kk) * 2);
        lso[i] = (uint32_t)(r * KROW + kk);
    }
    const uint32_t gtile = (uint32_t)(KVB * a.ld * 2);
    i32x4 sk[NS][NLD], sv[NS][NLD];
    auto gload = [&](int t) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NLD; ++i)
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                sk[s][i] = __builtin_amdgcn_raw_buffer_load_b128(rk[s], goff[i], t * gtile, 0);
                sv[s][i] = __builtin_amdgcn_raw_buffer_load_b128(rv[s], goff[i], t * gtile, 0);
            }
    };
    auto lstore = [&](int buf) __attribute__((always_inline)) {
        uint16_t *kd = smem + buf * TILE_E, *vd = kd + NS * KVB * KROW;
#pragma unroll
        for (int i = 0; i < NLD; ++i)
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                *reinterpret_cast<i32x4 *>(kd + s * KVB * KROW + lso[i]) = sk[s][i];
                *reinterpret_cast<i32x4 *>(vd + s * KVB * KROW + lso[i]) = sv[s][i];
            }
    };

    auto tile = [&](const uint16_t *Ks, const uint16_t *Vs, int t) __attribute__((always_inline)) {
        const int kleft = N - t * KVB;
        const int nkt = kleft >= KVB ? 4 : (kleft + 15) >> 4;      // 16-key sub-tiles holding a valid key
        f32x4 sc[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            sc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (kt < nkt) {
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const int kcol = c * 32 + g * 8;
                    const bf16x8 kh = *reinterpret_cast<const bf16x8 *>(Ks + (kt * 16 + l15) * KROW + kcol);
                    sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, qf[0][c], sc[kt], 0, 0, 0);
                    if (NSPLIT == 3) {
                        const bf16x8 kl = *reinterpret_cast<const bf16x8 *>(Ks + (KVB + kt * 16 + l15) * KROW + kcol);
                        sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, qf[NS - 1][c], sc[kt], 0, 0, 0);
                        sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl, qf[0][c], sc[kt], 0, 0, 0);
                    }
                }
            }
        }
        // exponent argument x = s * scale * log2(e) + (T_h + T_w)   (T already carries log2(e)); keys past N are masked
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = t * KVB + kt * 16 + g * 4 + r;
                const int kc = key < N ? key : N - 1;
                int ky, kx;
                coords(kc, ky, kx);
                const float bias = Th[-ky] + Tw[-kx];
                sc[kt][r] = key < N ? fmaf(sc[kt][r], cexp, bias) : -INFINITY;
            }
        float tmax = fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3]));
#pragma unroll
        for (int kt = 1; kt < 4; ++kt) tmax = fmaxf(fmaxf(fmaxf(tmax, sc[kt][0]), fmaxf(sc[kt][1], sc[kt][2])), sc[kt][3]);
        tmax = max_over_groups(tmax);
        const float m_new = fmaxf(m_run, tmax);          // finite: every tile holds at least one valid key
        const float alpha = fast_exp2(m_run - m_new);
        m_run = m_new;
        uint32_t pk[4][2], pkl[4][2];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            float p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) p[r] = fast_exp2(sc[kt][r] - m_new);
            pk[kt][0] = pack_bf16(p[0], p[1]);
            pk[kt][1] = pack_bf16(p[2], p[3]);
            if (NSPLIT == 3) {
                pkl[kt][0] = pack_bf16(p[0] - __uint_as_float(pk[kt][0] << 16), p[1] - __uint_as_float(pk[kt][0] & 0xffff0000u));
                pkl[kt][1] = pack_bf16(p[2] - __uint_as_float(pk[kt][1] << 16), p[3] - __uint_as_float(pk[kt][1] & 0xffff0000u));
            }
        }
#pragma unroll
        for (int n = 0; n <= ND; ++n) o[n] *= alpha;
        // O^T += V^T P^T : A = V^T[d][keys] via the transposing LDS read, B = P^T straight from the registers.
        // k index of step s2, element j of lane group g  <->  key (2 s2 + (j >> 2)) * 16 + 4 g + (j & 3)   (both operands)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            if (2 * s2 < nkt) {
                uint4 u = make_uint4(pk[2 * s2][0], pk[2 * s2][1], pk[2 * s2 + 1][0], pk[2 * s2 + 1][1]);
                const bf16x8 pf = *reinterpret_cast<bf16x8 *>(&u);
                bf16x8 pfl;
                if (NSPLIT == 3) {
                    uint4 ul = make_uint4(pkl[2 * s2][0], pkl[2 * s2][1], pkl[2 * s2 + 1][0], pkl[2 * s2 + 1][1]);
                    pfl = *reinterpret_cast<bf16x8 *>(&ul);
                }
                const uint16_t *vbase = Vs + ((2 * s2) * 16 + 4 * g + (l15 >> 2)) * KROW;
#pragma unroll
                for (int n = 0; n < ND; ++n) {
                    const uint16_t *va = vbase + n * 16 + 4 * (l15 & 3);
                    bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4 *)va);
                    bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4 *)(va + 16 * KROW));
                    const bf16x8 vh = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
                    o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, pf, o[n], 0, 0, 0);
                    if (NSPLIT == 3) {
                        bf16x4 w0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4 *)(va + KVB * KROW));
                        bf16x4 w1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4 *)(va + (KVB + 16) * KROW));
                        const bf16x8 vlo = __builtin_shufflevector(w0, w1, 0, 1, 2, 3, 4, 5, 6, 7);
                        o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, pfl, o[n], 0, 0, 0);
                        o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vlo, pf, o[n], 0, 0, 0);
                    }
                }
                o[ND] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pf, o[ND], 0, 0, 0);     // row sums: the ones-row of V^T
                if (NSPLIT == 3) o[ND] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pfl, o[ND], 0, 0, 0);
            }
        }
    };

    // K / V tiles: tile t + 1 is in flight (registers) while tile t is computed.  Two stages: it is written to the other LDS
    // buffer after the MFMAs of tile t, one barrier per tile (which also publishes T before the first tile).  One stage: a barrier
    // before the write (all waves are done with tile t - 1) and one after it.
    gload(0);
    if (STAGES == 2) {
        lstore(0);
        __syncthreads();
        for (int t = 0; t < n_tiles; ++t) {
            const int buf = t & 1;
            if (t + 1 < n_tiles) gload(t + 1);
            tile(smem + buf * TILE_E, smem + buf * TILE_E + NS * KVB * KROW, t);
            if (t + 1 < n_tiles) lstore(buf ^ 1);
            __syncthreads();
        }
    } else {
        for (int t = 0; t < n_tiles; ++t) {
            if (t > 0) __syncthreads();
            lstore(0);
            __syncthreads();
            if (t + 1 < n_tiles) gload(t + 1);
            tile(smem, smem + NS * KVB * KROW, t);
        }
    }

    // ---- write back: lane holds O[qi][n * 16 + g * 4 + r]; o[ND][*] = l ----
    if (qi >= N) return;
    const float l_run = o[ND][0];
    const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
    const int64_t oo = ((int64_t)b * N + qi) * a.ldo + (int64_t)h * DH;
#pragma unroll
    for (int n = 0; n < ND; ++n) {
        const int d0 = n * 16 + g * 4;
        float y[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] = o[n][r] * inv;
        const uint2 hv = make_uint2(pack_bf16(y[0], y[1]), pack_bf16(y[2], y[3]));
        *reinterpret_cast<uint2 *>(a.o + oo + d0) = hv;
        if (a.ol) {
            const uint2 lv = make_uint2(pack_bf16(y[0] - __uint_as_float(hv.x << 16), y[1] - __uint_as_float(hv.x & 0xffff0000u)),
                                        pack_bf16(y[2] - __uint_as_float(hv.y << 16), y[3] - __uint_as_float(hv.y & 0xffff0000u)));
            *reinterpret_cast<uint2 *>(a.ol + oo + d0) = lv;
        }
    }
}

LvqLdsOnce g_lds_relpos;

}  // namespace

extern "C" int lvq_attention_relpos_ok(int gh, int gw, int dh) { return dh == DH && gh >= 1 && gh <= 64 && gw >= 1 && gw <= 64; }

// what lvq_attention_relpos_bf16 launches for a grid (host only): K | V stages and dynamic LDS bytes, from the functions the launch uses
extern "C" int lvq_attention_relpos_plan(int gh, int gw, int precision, int *stages, size_t *lds_bytes) {
    if ((precision != 1 && precision != 3) || !stages || !lds_bytes) return LVQ_EINVAL;
    if (!lvq_attention_relpos_ok(gh, gw, DH)) return LVQ_EUNSUPPORTED;
    const bool split = precision == 3;
    *stages = rel_stages(gh, gw, split);
    *lds_bytes = rel_lds_bytes(gh, gw, split, *stages);
    return LVQ_OK;
}

// the fused kernel keeps its bias table in LDS: no workspace (the argument pair stays in the call for the family's convention)
extern "C" size_t lvq_attention_relpos_workspace_bytes(int batch, int n_heads, int gh, int gw, int dh, int precision) {
    (void)batch; (void)n_heads; (void)gh; (void)gw; (void)dh; (void)precision;
    return 0;
}

extern "C" int lvq_attention_relpos_bf16(const lvq_bf16 *qkv, const lvq_bf16 *qkv_lo, int64_t ld_qkv, const lvq_bf16 *rel_h,
                                         const lvq_bf16 *rel_h_lo, const lvq_bf16 *rel_w, const lvq_bf16 *rel_w_lo, int batch, int n_heads,
                                         int gh, int gw, int dh, float scale, lvq_bf16 *o, lvq_bf16 *o_lo, int64_t ldo, void *ws,
                                         size_t ws_bytes, lvq_stream_t stream) {
    if (batch <= 0 || n_heads <= 0 || gh <= 0 || gw <= 0 || dh <= 0 || !qkv || !rel_h || !rel_w || !o || !(scale > 0.f)) return LVQ_EINVAL;
    const bool split = qkv_lo != nullptr;
    if (split != (rel_h_lo != nullptr) || split != (rel_w_lo != nullptr) || (o_lo && !split)) return LVQ_EINVAL;
    if (!lvq_attention_relpos_ok(gh, gw, dh)) return LVQ_EUNSUPPORTED;
    const int64_t d = (int64_t)n_heads * dh, n = (int64_t)gh * gw;
    if (ld_qkv < 3 * d || ldo < d) return LVQ_EINVAL;
    if ((ld_qkv & 7) || (ldo & 3)) return LVQ_EUNSUPPORTED;
    if (((uintptr_t)qkv | (uintptr_t)qkv_lo | (uintptr_t)rel_h | (uintptr_t)rel_h_lo | (uintptr_t)rel_w | (uintptr_t)rel_w_lo) & 15) return LVQ_EUNSUPPORTED;
    if (((uintptr_t)o | (uintptr_t)o_lo) & 7) return LVQ_EUNSUPPORTED;
    // one (batch, head) K / V slab is addressed with 32-bit buffer offsets
    if (((n + KVB) * ld_qkv + dh) * 2 >= (1ll << 32)) return LVQ_EUNSUPPORTED;
    const int nqt = (int)lvq_cdiv(n, NW * 16);
    const int64_t nwg = (int64_t)batch * n_heads * nqt;
    if (nwg > 0x7fffffff) return LVQ_EUNSUPPORTED;
    if (ws_bytes < lvq_attention_relpos_workspace_bytes(batch, n_heads, gh, gw, dh, split ? 3 : 1)) return LVQ_EWORKSPACE;
    (void)ws;
    // the family's largest request (two stages, hi + lo, a grid whose waves span rows), set once per device
    if (!lvq_ensure_lds(g_lds_relpos, {(const void *)k_attn_relpos<1, 1>, (const void *)k_attn_relpos<1, 2>, (const void *)k_attn_relpos<3, 1>,
                                       (const void *)k_attn_relpos<3, 2>}, rel_lds_max()))
        return LVQ_ELAUNCH;
    RelArgs a{};
    a.qkv = qkv; a.qkvl = qkv_lo; a.rh = rel_h; a.rhl = rel_h_lo; a.rw = rel_w; a.rwl = rel_w_lo;
    a.B = batch; a.H = n_heads; a.gh = gh; a.gw = gw; a.nqt = nqt; a.ts = rel_tab_stride(gh, gw); a.ld = ld_qkv; a.ldo = ldo; a.scale = scale; a.o = o; a.ol = o_lo;
    hipStream_t st = lvq_s(stream);
    const int stages = rel_stages(gh, gw, split);
    const size_t l = rel_lds_bytes(gh, gw, split, stages);
    if (split && stages == 1)      hipLaunchKernelGGL((k_attn_relpos<3, 1>), dim3((unsigned)nwg), dim3(NT), l, st, a);
    else if (split)                hipLaunchKernelGGL((k_attn_relpos<3, 2>), dim3((unsigned)nwg), dim3(NT), l, st, a);
    else if (stages == 1)          hipLaunchKernelGGL((k_attn_relpos<1, 1>), dim3((unsigned)nwg), dim3(NT), l, st, a);
    else                           hipLaunchKernelGGL((k_attn_relpos<1, 2>), dim3((unsigned)nwg), dim3(NT), l, st, a);
    return lvq_launch_status();
}
