// csrc/decode_ragged.hip -- one decode step of a RAGGED batch: every sequence has its own position.
//
//   k_decode_ragged        attention of one query token per sequence over kv_len[b] cached keys (a device array).  Work unit =
//                          (sequence, KV head, chunk of RCHUNK keys), one wave.  The n_heads / n_kv_heads query heads that share the
//                          KV head are the columns of ONE 16-wide MFMA tile (zero-padded), so a K / V row is loaded once and serves
//                          the whole group; the generic tile kernel (attention.hip) spends a tile per query head with 15 idle columns
//                          and reads the row once per head.  K goes from global memory straight into the A-operand registers
//                          (S^T = K Q^T, as in attention.hip); V passes through LDS once for the transposing read of O^T = V^T P^T.
//   k_decode_ragged_merge  merges the chunk partials (unnormalised O | m | l) of a sequence in ascending chunk order.
//   k_rope_cache_ragged    decoder.hip's k_rope_cache with the position pos0[b] + t.
//
// The chunk length is a compile-time constant and a sequence's work units depend on its own kv_len only -- not on the batch size,
// the other sequences or the tuning record -- so the output row of a sequence has the same bits in every batch.  kv_len is read on the
// device: no host read, no synchronisation.
#include "decode_common.h"

namespace {

constexpr int RKVB = LVQ_RKVB;
constexpr int RCHUNK = LVQ_RCHUNK;      // keys per work unit: FIXED (see above)

struct RaggedArgs {
    const uint16_t *q, *ql, *k, *kl, *v, *vl;
    const int32_t *kv_len;
    int B, H, Hkv, lmax, dh, nchunk;
    int64_t q_bs, q_hs, k_bs, ldk, k_hs, v_bs, ldv, v_hs, o_bs, o_hs;
    float scale;
    uint16_t *o, *ol;
    float *part;                // [B][H][nchunk][DHP + 4] fp32: unnormalised O (DHP) | m (log2 domain) | l | pad
};

__device__ __forceinline__ int clamp_len(int len, int lmax) { return len < 0 ? 0 : (len > lmax ? lmax : len); }

// DHP = padded head dim (64 or 128), NS = operand parts (1: plain bf16, 2: hi + lo -> three MFMA passes, the bf16x3 mode)
template <int DHP, int NS>
__global__ void __launch_bounds__(64) k_decode_ragged(RaggedArgs a) {
    constexpr int NC = DHP / 32;        // 32-wide k chunks of the head dim
    constexpr int ND = DHP / 16;        // 16-wide output tiles of the head dim
    constexpr int KROW = DHP + 8;       // bf16 elements per V row in LDS (the padding of attention.hip's unswizzled form)
    constexpr int CH = DHP / 8;         // 16-byte pieces per row
    __shared__ __attribute__((aligned(16))) uint16_t Vs[NS * RKVB * KROW];

    const int c = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
    const int len = clamp_len(a.kv_len[b], a.lmax);
    const int k0 = c * RCHUNK;
    if (k0 >= len) return;                                   // a work unit past the sequence's length (len == 0: all of them)
    const int k1 = len < k0 + RCHUNK ? len : k0 + RCHUNK;    // keys k0 .. k1-1; rows from k1 on are never loaded
    const int lane = threadIdx.x, g = lane >> 4, l15 = lane & 15;
    const int G = a.H / a.Hkv, h = hk * G + l15;             // this lane's query head (column l15 of the tile), valid when l15 < G
    const float cexp = a.scale * 1.4426950408889634f;        // scores are exponentiated in the log2 domain

    // Q fragments (B operand of S^T = K Q^T): lane supplies Q[head h][c*32 + 8g .. +7]; columns G .. 15 are zero
    bf16x8 qf[NS][NC];
    {
        const uint16_t *src[2] = {a.q, a.ql};
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) {
                const int kk = cc * 32 + g * 8;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (l15 < G && kk < a.dh) v = *reinterpret_cast<const uint4 *>(src[s] + (int64_t)b * a.q_bs + (int64_t)h * a.q_hs + kk);
                qf[s][cc] = __builtin_bit_cast(bf16x8, v);
            }
    }
    const uint16_t *kb[2] = {a.k + (int64_t)b * a.k_bs + (int64_t)hk * a.k_hs, a.kl ? a.kl + (int64_t)b * a.k_bs + (int64_t)hk * a.k_hs : nullptr};
    const uint16_t *vb[2] = {a.v + (int64_t)b * a.v_bs + (int64_t)hk * a.v_hs, a.vl ? a.vl + (int64_t)b * a.v_bs + (int64_t)hk * a.v_hs : nullptr};

    // o[ND] is the row-sum tile: V^T is extended by a row of ones, so l = sum_j p_j falls out of the same MFMAs
    f32x4 o[ND + 1];
#pragma unroll
    for (int n = 0; n <= ND; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY;
    bf16x8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (short)0x3F80;

    for (int t0 = k0; t0 < k1; t0 += RKVB) {                 // every tile holds at least one valid key
        // K fragments (A operand): lane supplies K[key t0 + kt*16 + l15][c*32 + 8g .. +7]; rows from k1 on and head-dim padding read as zero
        bf16x8 kf[NS][4][NC];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const int key = t0 + kt * 16 + l15;
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) {
                const int kk = cc * 32 + g * 8;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    uint4 v = make_uint4(0, 0, 0, 0);
                    if (key < k1 && kk < a.dh) v = *reinterpret_cast<const uint4 *>(kb[s] + (int64_t)key * a.ldk + kk);
                    kf[s][kt][cc] = __builtin_bit_cast(bf16x8, v);
                }
            }
        }
        // V rows of the tile: piece e = lane + 64 i is columns 8 (e % CH) .. +7 of row e / CH; same zero fill
        uint4 vr[NS][CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int e = lane + 64 * i, r = e / CH, kk = (e - r * CH) * 8;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                vr[s][i] = make_uint4(0, 0, 0, 0);
                if (t0 + r < k1 && kk < a.dh) vr[s][i] = *reinterpret_cast<const uint4 *>(vb[s] + (int64_t)(t0 + r) * a.ldv + kk);
            }
        }

        // S^T = K Q^T: sc[kt][r] = score of key t0 + kt*16 + 4g + r for query head l15
        f32x4 sc[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            sc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) {
                sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[0][kt][cc], qf[0][cc], sc[kt], 0, 0, 0);
                if (NS == 2) {
                    sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[0][kt][cc], qf[NS - 1][cc], sc[kt], 0, 0, 0);
                    sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[NS - 1][kt][cc], qf[0][cc], sc[kt], 0, 0, 0);
                }
            }
        }
        float tmax = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = t0 + kt * 16 + g * 4 + r;
                sc[kt][r] = key < k1 ? sc[kt][r] * cexp : -INFINITY;
                tmax = fmaxf(tmax, sc[kt][r]);
            }
        tmax = max_over_groups(tmax);
        const float m_new = fmaxf(m_run, tmax);
        const float m_safe = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = exp2f(m_run - m_safe);           // first tile: exp2(-inf) = 0 on zero accumulators
        m_run = m_new;
        uint32_t pk[4][2], pkl[4][2];                        // packed bf16 P^T [kt][pair], hi and (hi + lo mode) lo parts
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            float p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) p[r] = exp2f(sc[kt][r] - m_safe);
            pk[kt][0] = pack_bf16(p[0], p[1]);
            pk[kt][1] = pack_bf16(p[2], p[3]);
            if (NS == 2) {
                pkl[kt][0] = pack_bf16(p[0] - __uint_as_float(pk[kt][0] << 16), p[1] - __uint_as_float(pk[kt][0] & 0xffff0000u));
                pkl[kt][1] = pack_bf16(p[2] - __uint_as_float(pk[kt][1] << 16), p[3] - __uint_as_float(pk[kt][1] & 0xffff0000u));
            }
        }
#pragma unroll
        for (int n = 0; n <= ND; ++n) o[n] *= alpha;

        __syncthreads();                                     // the previous tile's reads of Vs are done
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int e = lane + 64 * i, r = e / CH, kk = (e - r * CH) * 8;
#pragma unroll
            for (int s = 0; s < NS; ++s) *reinterpret_cast<uint4 *>(Vs + (s * RKVB + r) * KROW + kk) = vr[s][i];
        }
        __syncthreads();

        // O^T += V^T P^T : A = V^T[d][keys] via the transposing LDS read, B = P^T straight from the registers.
        // k index of step s2, element j of lane group g  <->  key (2*s2 + (j>>2))*16 + 4g + (j&3)   (both operands)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const uint4 u = make_uint4(pk[2 * s2][0], pk[2 * s2][1], pk[2 * s2 + 1][0], pk[2 * s2 + 1][1]);
            const bf16x8 pf = __builtin_bit_cast(bf16x8, u);
            bf16x8 pfl;
            if (NS == 2) {
                const uint4 ul = make_uint4(pkl[2 * s2][0], pkl[2 * s2][1], pkl[2 * s2 + 1][0], pkl[2 * s2 + 1][1]);
                pfl = __builtin_bit_cast(bf16x8, ul);
            }
            // lane 4q+p of a 16-lane group addresses row q, columns 4p..4p+3 of its group's 4-key x 16-d block
            const uint16_t *vbase = Vs + ((2 * s2) * 16 + 4 * g + (l15 >> 2)) * KROW;
#pragma unroll
            for (int n = 0; n < ND; ++n) {
                const uint16_t *va = vbase + n * 16 + 4 * (l15 & 3);
                const bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4 *)va);
                const bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4 *)(va + 16 * KROW));
                const bf16x8 vh = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
                o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, pf, o[n], 0, 0, 0);
                if (NS == 2) {
                    const bf16x4 w0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4 *)(va + RKVB * KROW));
                    const bf16x4 w1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4 *)(va + (RKVB + 16) * KROW));
                    const bf16x8 vlo = __builtin_shufflevector(w0, w1, 0, 1, 2, 3, 4, 5, 6, 7);
                    o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vh, pfl, o[n], 0, 0, 0);
                    o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vlo, pf, o[n], 0, 0, 0);
                }
            }
            o[ND] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pf, o[ND], 0, 0, 0);
            if (NS == 2) o[ND] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pfl, o[ND], 0, 0, 0);
        }
    }

    // partial of this chunk: lane holds O[head l15][n*16 + 4g + r]; o[ND][*] = l
    if (l15 < G) {
        float *pr = a.part + (((int64_t)b * a.H + h) * a.nchunk + c) * (DHP + 4);
#pragma unroll
        for (int n = 0; n < ND; ++n) *reinterpret_cast<f32x4 *>(pr + n * 16 + g * 4) = o[n];
        if (g == 0) { pr[DHP] = m_run; pr[DHP + 1] = o[ND][0]; }
    }
}

// one thread per (sequence, head, output element): the chunk partials merged in ascending chunk order; a sequence of length 0 gets zeros
__global__ void __launch_bounds__(128) k_decode_ragged_merge(RaggedArgs a, int dhp) {
    const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
    if (d >= a.dh) return;
    const int len = clamp_len(a.kv_len[b], a.lmax);
    const int n = (len + RCHUNK - 1) / RCHUNK;
    const float *pr = a.part + (((int64_t)b * a.H + h) * a.nchunk) * (dhp + 4);
    float m = -INFINITY, l = 0.f, acc = 0.f;
    for (int c = 0; c < n; ++c, pr += dhp + 4) {
        const float mc = pr[dhp], lc = pr[dhp + 1], oc = pr[d];
        const float mn = fmaxf(m, mc);
        const float ms = mn == -INFINITY ? 0.f : mn;
        const float a1 = exp2f(m - ms), a2 = exp2f(mc - ms);
        acc = acc * a1 + oc * a2;
        l = l * a1 + lc * a2;
        m = mn;
    }
    const float y = l > 0.f ? acc / l : 0.f;
    const int64_t at = (int64_t)b * a.o_bs + (int64_t)h * a.o_hs + d;
    const uint16_t hi = f32_to_bf16(y);
    a.o[at] = hi;
    if (a.ol) a.ol[at] = f32_to_bf16(y - bf16_to_f32(hi));
}

__global__ void __launch_bounds__(256) k_rope_cache_ragged(uint16_t *__restrict__ xh, uint16_t *__restrict__ xl, int batch, int n_heads, int n_kv_heads,
                                                           int dh, const int32_t *__restrict__ pos0, int t, int lmax, float theta,
                                                           uint16_t *__restrict__ kc, uint16_t *__restrict__ kcl, uint16_t *__restrict__ vc,
                                                           uint16_t *__restrict__ vcl, int32_t *__restrict__ kv_len) {
    const int per_row = (n_heads + n_kv_heads) * (dh >> 1) + n_kv_heads * dh;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= batch * per_row) return;
    const int b = i / per_row, j = i - b * per_row;
    // a sequence that has run out of cache rows keeps overwriting its last row instead of writing outside its cache
    const int64_t want = (int64_t)pos0[b] + t;
    const int pos = want < 0 ? 0 : (want > lmax - 1 ? lmax - 1 : (int)want);
    if (j == 0 && kv_len) kv_len[b] = pos + 1;
    lvq_rope_cache_item(xh, xl, b, j, n_heads, n_kv_heads, dh, pos, lmax, theta, kc, kcl, vc, vcl);
}

bool shape_ok(int batch, int n_heads, int n_kv_heads, int lmax, int dh, int precision) {
    return batch > 0 && batch <= 65535 && n_heads > 0 && n_kv_heads > 0 && n_kv_heads <= 65535 && n_heads % n_kv_heads == 0 &&
           n_heads / n_kv_heads <= 16 && lmax > 0 && dh > 0 && dh % 16 == 0 && dh <= 128 && (precision == 1 || precision == 3);
}
inline int padded_dh(int dh) { return dh <= 64 ? 64 : 128; }
inline bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

void lvq_rope_cache_ragged(uint16_t *xh, uint16_t *xl, int batch, int n_heads, int n_kv_heads, int dh, const int32_t *pos0, int t, int lmax,
                           float theta, uint16_t *kc, uint16_t *kcl, uint16_t *vc, uint16_t *vcl, int32_t *kv_len, hipStream_t st) {
    const int per_row = (n_heads + n_kv_heads) * (dh / 2) + n_kv_heads * dh;
    hipLaunchKernelGGL(k_rope_cache_ragged, dim3((unsigned)lvq_cdiv((int64_t)batch * per_row, 256)), dim3(256), 0, st, xh, xl, batch, n_heads,
                       n_kv_heads, dh, pos0, t, lmax, theta, kc, kcl, vc, vcl, kv_len);
}

extern "C" size_t lvq_attention_decode_ragged_workspace_bytes(int batch, int n_heads, int n_kv_heads, int lmax, int dh, int precision) {
    if (!shape_ok(batch, n_heads, n_kv_heads, lmax, dh, precision)) return 0;
    LvqSizer s;
    s.take<float>((size_t)batch * n_heads * (size_t)lvq_cdiv(lmax, RCHUNK) * (padded_dh(dh) + 4));
    return s.total();
}

extern "C" int lvq_attention_decode_ragged(const lvq_bf16 *q, const lvq_bf16 *q_lo, const lvq_bf16 *k_cache, const lvq_bf16 *k_cache_lo,
                                           const lvq_bf16 *v_cache, const lvq_bf16 *v_cache_lo, const int32_t *kv_len, int batch, int n_heads,
                                           int n_kv_heads, int lmax, int dh, int64_t q_bstride, int64_t ldq, int64_t q_hstride, int64_t k_bstride,
                                           int64_t ldk, int64_t k_hstride, int64_t v_bstride, int64_t ldv, int64_t v_hstride, int64_t o_bstride,
                                           int64_t ldo, int64_t o_hstride, float scale, lvq_bf16 *o, lvq_bf16 *o_lo, void *ws, size_t ws_bytes,
                                           lvq_stream_t stream) {
    (void)ldq; (void)ldo;                                    // one query row per sequence: the row strides of lvq_attention_bf16 have nothing to step over
    const bool x3 = q_lo != nullptr;
    if (!q || !k_cache || !v_cache || !kv_len || !o || !shape_ok(batch, n_heads, n_kv_heads, lmax, dh, x3 ? 3 : 1) || !(scale > 0.f))
        return LVQ_EINVAL;
    if (x3 != (k_cache_lo != nullptr) || x3 != (v_cache_lo != nullptr)) return LVQ_EINVAL;     // plain, or hi + lo on all three operands
    // 16-byte vector loads: every operand row starts on a 16-byte boundary
    for (int64_t s : {q_bstride, q_hstride, k_bstride, ldk, k_hstride, v_bstride, ldv, v_hstride})
        if (s < 0 || s % 8) return LVQ_EINVAL;
    if (o_bstride < 0 || o_hstride < 0) return LVQ_EINVAL;
    for (const void *p : {(const void *)q, (const void *)q_lo, (const void *)k_cache, (const void *)k_cache_lo, (const void *)v_cache, (const void *)v_cache_lo})
        if (!al16(p)) return LVQ_EINVAL;
    const int dhp = padded_dh(dh);
    LvqArena arena(ws, ws_bytes);
    RaggedArgs a;
    a.nchunk = (int)lvq_cdiv(lmax, RCHUNK);
    a.part = arena.take<float>((size_t)batch * n_heads * (size_t)a.nchunk * (dhp + 4));
    if (!arena.ok || !al16(a.part)) return LVQ_EWORKSPACE;
    a.q = q; a.ql = q_lo; a.k = k_cache; a.kl = k_cache_lo; a.v = v_cache; a.vl = v_cache_lo;
    a.kv_len = kv_len;
    a.B = batch; a.H = n_heads; a.Hkv = n_kv_heads; a.lmax = lmax; a.dh = dh;
    a.q_bs = q_bstride; a.q_hs = q_hstride; a.k_bs = k_bstride; a.ldk = ldk; a.k_hs = k_hstride;
    a.v_bs = v_bstride; a.ldv = ldv; a.v_hs = v_hstride; a.o_bs = o_bstride; a.o_hs = o_hstride;
    a.scale = scale; a.o = o; a.ol = o_lo;
    hipStream_t st = lvq_s(stream);
    const dim3 grid((unsigned)a.nchunk, (unsigned)n_kv_heads, (unsigned)batch);
    if (dhp == 64) {
        if (x3) hipLaunchKernelGGL((k_decode_ragged<64, 2>), grid, dim3(64), 0, st, a);
        else hipLaunchKernelGGL((k_decode_ragged<64, 1>), grid, dim3(64), 0, st, a);
    } else {
        if (x3) hipLaunchKernelGGL((k_decode_ragged<128, 2>), grid, dim3(64), 0, st, a);
        else hipLaunchKernelGGL((k_decode_ragged<128, 1>), grid, dim3(64), 0, st, a);
    }
    hipLaunchKernelGGL(k_decode_ragged_merge, dim3((unsigned)n_heads, (unsigned)batch), dim3(128), 0, st, a, dhp);
    return lvq_launch_status();
}
