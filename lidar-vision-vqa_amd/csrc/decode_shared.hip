// csrc/decode_shared.hip -- attention of sequences that continue a SHARED, read-only prefix (many questions about one scene).
//
// Sequence b belongs to prefix g = prefix_index[b].  Its history is the plen[g] rows of that prefix cache [G, pmax, dkv] followed by the
// rows of its own cache [B, lown, dkv]; nothing is copied: a key at global position p comes from the prefix cache when p < plen[g] and
// from own row p - plen[g] otherwise.  The sequence brings qn[b] >= 1 query rows (the question prefill: qn = question length, a decode
// step: qn = 1) behind `own` rows that are already cached; query row r stands at global position plen[g] + own + r and sees the keys
// up to and including its own.
//
//   k_extend_shared        decode_ragged.hip's k_decode_ragged with two changes.  The columns of the 16-wide MFMA tile are the
//                          (query row, query head) pairs of one KV head, n_heads / n_kv_heads heads per row, tile after tile; every
//                          column has its own key limit (causality inside the chunk of query rows).  And the K / V row pointer is
//                          chosen per key between the two caches.  Work unit = (sequence, KV head, column tile, chunk of LVQ_RCHUNK
//                          keys), one wave; the chunks are cut at GLOBAL positions.
//   k_extend_shared_merge  merges the chunk partials of one (sequence, query row, head) in ascending chunk order; rows r >= qn[b] get zeros.
//   k_rope_cache_shared    rotary at the global position, append to the own cache, for r < qn[b] only.
//
// With qn = 1 a sequence has the keys in the lanes, tiles and chunks k_decode_ragged gives it on a cache that holds prefix and own rows
// one behind the other, and the same arithmetic: bit-identical output.  A sequence's work units depend on its own lengths only -- not on
// the batch, its slot or its neighbours.  All lengths are read on the device: no host read, no synchronisation.  Rows behind a length
// are never loaded.  (A tile that shares prefix loads ACROSS sequences is deliberately not built: DESIGN 3.4 / 3.5.)
#include "decode_common.h"

namespace {

constexpr int RKVB = LVQ_RKVB;
constexpr int RCHUNK = LVQ_RCHUNK;

struct SharedArgs {
    const uint16_t *q, *ql, *pk, *pkl, *pv, *pvl, *k, *kl, *v, *vl;
    const int32_t *pidx, *plen, *own0, *qn;
    const int4 *lens;           // != nullptr: (g, plen, own, qn) per sequence, already clamped (k_rope_cache_shared wrote it) -- ONE load per
                                // wave instead of the dependent pair prefix_index[b] -> plen[g]; the four arrays are then unused
    int B, Lq, H, Hkv, n_prefix, pmax, lown, dh, nchunk, ntile;
    int64_t q_bs, ldq, q_hs, pk_bs, k_bs, ldk, k_hs, pv_bs, v_bs, ldv, v_hs, o_bs, ldo, o_hs;
    float scale;
    uint16_t *o, *ol;
    float *part;                // [B][Lq][H][nchunk][DHP + 4] fp32: unnormalised O (DHP) | m (log2 domain) | l | pad
};

__device__ __forceinline__ int clampi(int64_t x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : (int)x); }

// the lengths of sequence b, clamped to what the buffers hold
struct SeqLens {
    int g, plen, own, qn;
    // number of keys query row r sees: the prefix, the cached own rows and the query rows up to r; never more own rows than the cache has
    __device__ __forceinline__ int keys(int r, int lown) const {
        const int o = own + r + 1;
        return plen + (o < lown ? o : lown);
    }
};
__device__ __forceinline__ SeqLens seq_lens(const int32_t *pidx, const int32_t *plen, const int32_t *own0, const int32_t *qn, int t, int b, int n_prefix,
                                            int pmax, int lown, int lq) {
    SeqLens s;
    s.g = clampi(pidx[b], 0, n_prefix - 1);
    s.plen = clampi(plen[s.g], 0, pmax);
    s.own = clampi((int64_t)own0[b] + t, 0, lown);
    s.qn = clampi(qn[b], 0, lq);
    return s;
}

__device__ __forceinline__ SeqLens seq_lens(const SharedArgs &a, int b) {
    if (a.lens) {
        const int4 v = a.lens[b];
        SeqLens s;
        s.g = v.x; s.plen = v.y; s.own = v.z; s.qn = v.w;
        return s;
    }
    return seq_lens(a.pidx, a.plen, a.own0, a.qn, 0, b, a.n_prefix, a.pmax, a.lown, a.Lq);
}

// DHP = padded head dim (64 or 128), NS = operand parts (1: plain bf16, 2: hi + lo -> three MFMA passes, the bf16x3 mode)
template <int DHP, int NS>
__global__ void __launch_bounds__(64) k_extend_shared(SharedArgs a) {
    constexpr int NC = DHP / 32;        // 32-wide k chunks of the head dim
    constexpr int ND = DHP / 16;        // 16-wide output tiles of the head dim
    constexpr int KROW = DHP + 8;       // bf16 elements per V row in LDS (the padding of attention.hip's unswizzled form)
    constexpr int CH = DHP / 8;         // 16-byte pieces per row
    __shared__ __attribute__((aligned(16))) uint16_t Vs[NS * RKVB * KROW];

    const int c = blockIdx.x, b = blockIdx.z;
    const int hk = blockIdx.y / a.ntile, tile = blockIdx.y - hk * a.ntile;
    const SeqLens s = seq_lens(a, b);
    const int G = a.H / a.Hkv;
    if ((tile * 16) / G >= s.qn) return;                     // a column tile behind the sequence's query rows
    int r_hi = (tile * 16 + 15) / G;                         // last query row with a column in this tile
    if (r_hi > s.qn - 1) r_hi = s.qn - 1;
    const int kend = s.keys(r_hi, a.lown);                   // keys of the tile's last row: the other rows see fewer
    const int k0 = c * RCHUNK;
    if (k0 >= kend) return;                                  // a work unit past the keys of this tile
    const int k1 = kend < k0 + RCHUNK ? kend : k0 + RCHUNK;  // keys k0 .. k1-1; rows from k1 on are never loaded
    const int lane = threadIdx.x, g = lane >> 4, l15 = lane & 15;
    const int col = tile * 16 + l15, r = col / G, h = hk * G + (col - r * G);     // this lane's (query row, query head)
    const bool live = r < s.qn;
    const int klim = live ? s.keys(r, a.lown) : 0;           // this column's own key limit
    const float cexp = a.scale * 1.4426950408889634f;        // scores are exponentiated in the log2 domain

    // Q fragments (B operand of S^T = K Q^T): lane supplies Q[row r, head h][c*32 + 8g .. +7]; dead columns are zero
    bf16x8 qf[NS][NC];
    {
        const uint16_t *src[2] = {a.q, a.ql};
#pragma unroll
        for (int p = 0; p < NS; ++p)
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) {
                const int kk = cc * 32 + g * 8;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (live && kk < a.dh)
                    v = *reinterpret_cast<const uint4 *>(src[p] + (int64_t)b * a.q_bs + (int64_t)r * a.ldq + (int64_t)h * a.q_hs + kk);
                qf[p][cc] = __builtin_bit_cast(bf16x8, v);
            }
    }
    // row 0 of this KV head in the group's prefix cache and in the sequence's own cache
    const int64_t pko = (int64_t)s.g * a.pk_bs + (int64_t)hk * a.k_hs, oko = (int64_t)b * a.k_bs + (int64_t)hk * a.k_hs;
    const int64_t pvo = (int64_t)s.g * a.pv_bs + (int64_t)hk * a.v_hs, ovo = (int64_t)b * a.v_bs + (int64_t)hk * a.v_hs;
    const uint16_t *pkb[2] = {a.pk + pko, a.pkl ? a.pkl + pko : nullptr}, *okb[2] = {a.k + oko, a.kl ? a.kl + oko : nullptr};
    const uint16_t *pvb[2] = {a.pv + pvo, a.pvl ? a.pvl + pvo : nullptr}, *ovb[2] = {a.v + ovo, a.vl ? a.vl + ovo : nullptr};

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
            const bool pre = key < s.plen;
            const int64_t ro = pre ? (int64_t)key * a.ldk : (int64_t)(key - s.plen) * a.ldk;
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) {
                const int kk = cc * 32 + g * 8;
#pragma unroll
                for (int p = 0; p < NS; ++p) {
                    uint4 v = make_uint4(0, 0, 0, 0);
                    if (key < k1 && kk < a.dh) v = *reinterpret_cast<const uint4 *>((pre ? pkb[p] : okb[p]) + ro + kk);
                    kf[p][kt][cc] = __builtin_bit_cast(bf16x8, v);
                }
            }
        }
        // V rows of the tile: piece e = lane + 64 i is columns 8 (e % CH) .. +7 of row e / CH; same zero fill
        uint4 vr[NS][CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int e = lane + 64 * i, rr = e / CH, kk = (e - rr * CH) * 8;
            const int key = t0 + rr;
            const bool pre = key < s.plen;
            const int64_t ro = pre ? (int64_t)key * a.ldv : (int64_t)(key - s.plen) * a.ldv;
#pragma unroll
            for (int p = 0; p < NS; ++p) {
                vr[p][i] = make_uint4(0, 0, 0, 0);
                if (key < k1 && kk < a.dh) vr[p][i] = *reinterpret_cast<const uint4 *>((pre ? pvb[p] : ovb[p]) + ro + kk);
            }
        }

        // S^T = K Q^T: sc[kt][i] = score of key t0 + kt*16 + 4g + i for column l15
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
            for (int i = 0; i < 4; ++i) {
                const int key = t0 + kt * 16 + g * 4 + i;
                sc[kt][i] = key < klim ? sc[kt][i] * cexp : -INFINITY;       // the column's own limit: causal inside the query chunk
                tmax = fmaxf(tmax, sc[kt][i]);
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
            for (int i = 0; i < 4; ++i) p[i] = exp2f(sc[kt][i] - m_safe);
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
            const int e = lane + 64 * i, rr = e / CH, kk = (e - rr * CH) * 8;
#pragma unroll
            for (int p = 0; p < NS; ++p) *reinterpret_cast<uint4 *>(Vs + (p * RKVB + rr) * KROW + kk) = vr[p][i];
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

    // partial of this chunk: lane holds O[column l15][n*16 + 4g + i]; o[ND][*] = l
    if (live) {
        float *pr = a.part + ((((int64_t)b * a.Lq + r) * a.H + h) * a.nchunk + c) * (DHP + 4);
#pragma unroll
        for (int n = 0; n < ND; ++n) *reinterpret_cast<f32x4 *>(pr + n * 16 + g * 4) = o[n];
        if (g == 0) { pr[DHP] = m_run; pr[DHP + 1] = o[ND][0]; }
    }
}

// one thread per (sequence, query row, head, output element): the chunk partials merged in ascending chunk order; rows r >= qn[b] get zeros
__global__ void __launch_bounds__(128) k_extend_shared_merge(SharedArgs a, int dhp) {
    const int h = blockIdx.x, r = blockIdx.y, b = blockIdx.z, d = threadIdx.x;
    if (d >= a.dh) return;
    const SeqLens s = seq_lens(a, b);
    const int n = r < s.qn ? (s.keys(r, a.lown) + RCHUNK - 1) / RCHUNK : 0;
    const float *pr = a.part + ((((int64_t)b * a.Lq + r) * a.H + h) * a.nchunk) * (dhp + 4);
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
    const int64_t at = (int64_t)b * a.o_bs + (int64_t)r * a.ldo + (int64_t)h * a.o_hs + d;
    const uint16_t hi = f32_to_bf16(y);
    a.o[at] = hi;
    if (a.ol) a.ol[at] = f32_to_bf16(y - bf16_to_f32(hi));
}

__global__ void __launch_bounds__(256) k_rope_cache_shared(uint16_t *__restrict__ xh, uint16_t *__restrict__ xl, int batch, int lq, int n_heads,
                                                           int n_kv_heads, int dh, const int32_t *__restrict__ pidx,
                                                           const int32_t *__restrict__ plen, int n_prefix, int pmax,
                                                           const int32_t *__restrict__ own0, const int32_t *__restrict__ qn, int t, int lown,
                                                           float theta, uint16_t *__restrict__ kc, uint16_t *__restrict__ kcl,
                                                           uint16_t *__restrict__ vc, uint16_t *__restrict__ vcl, const int4 *__restrict__ lens_in,
                                                           int4 *__restrict__ lens_out) {
    const int per_row = (n_heads + n_kv_heads) * (dh >> 1) + n_kv_heads * dh;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)batch * lq * per_row) return;
    const int64_t row = i / per_row;                         // packed row b * lq + r
    const int j = (int)(i - row * per_row), b = (int)(row / lq), r = (int)(row - (int64_t)b * lq);
    SeqLens s;
    if (lens_in) {                                           // what an earlier layer of this step left: one load
        const int4 v = lens_in[b];
        s.g = v.x; s.plen = v.y; s.own = v.z; s.qn = v.w;
    } else {
        s = seq_lens(pidx, plen, own0, qn, t, b, n_prefix, pmax, lown, lq);
        if (r == 0 && j == 0 && lens_out) lens_out[b] = make_int4(s.g, s.plen, s.own, s.qn);     // for the launches behind this one
    }
    if (r >= s.qn) return;                                   // a padding row: nothing is rotated, nothing is appended
    // a sequence that has run out of own cache rows keeps overwriting its last row instead of writing outside its cache
    const int own = s.own + r < lown - 1 ? s.own + r : lown - 1;
    lvq_rope_cache_item_at(xh, xl, row, j, n_heads, n_kv_heads, dh, s.plen + own, (int64_t)b * lown + own, theta, kc, kcl, vc, vcl);
}

bool shape_ok(int batch, int lq, int n_heads, int n_kv_heads, int n_prefix, int pmax, int lown, int dh, int precision) {
    if (!(batch > 0 && batch <= 65535 && lq > 0 && lq <= 65535 && n_heads > 0 && n_kv_heads > 0 && n_heads % n_kv_heads == 0 &&
          n_heads / n_kv_heads <= 16 && n_prefix > 0 && pmax > 0 && lown > 0 && dh > 0 && dh % 16 == 0 && dh <= 128 &&
          (precision == 1 || precision == 3)))
        return false;
    if ((int64_t)pmax + lown > (int64_t)1 << 30) return false;
    return n_kv_heads * lvq_cdiv((int64_t)lq * (n_heads / n_kv_heads), 16) <= 65535;       // grid.y
}
inline int padded_dh(int dh) { return dh <= 64 ? 64 : 128; }
inline bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

void lvq_rope_cache_shared(uint16_t *xh, uint16_t *xl, int batch, int lq, int n_heads, int n_kv_heads, int dh, const int32_t *prefix_index,
                           const int32_t *plen, int n_prefix, int pmax, const int32_t *own0, const int32_t *qn, int t, int lown, float theta,
                           uint16_t *kc, uint16_t *kcl, uint16_t *vc, uint16_t *vcl, const int4 *lens_in, int4 *lens_out, hipStream_t st) {
    const int per_row = (n_heads + n_kv_heads) * (dh / 2) + n_kv_heads * dh;
    hipLaunchKernelGGL(k_rope_cache_shared, dim3((unsigned)lvq_cdiv((int64_t)batch * lq * per_row, 256)), dim3(256), 0, st, xh, xl, batch, lq,
                       n_heads, n_kv_heads, dh, prefix_index, plen, n_prefix, pmax, own0, qn, t, lown, theta, kc, kcl, vc, vcl, lens_in, lens_out);
}

extern "C" size_t lvq_attention_extend_shared_workspace_bytes(int batch, int lq, int n_heads, int n_kv_heads, int pmax, int lown, int dh,
                                                              int precision) {
    if (!shape_ok(batch, lq, n_heads, n_kv_heads, 1, pmax, lown, dh, precision)) return 0;
    LvqSizer s;
    s.take<float>((size_t)batch * lq * n_heads * (size_t)lvq_cdiv((int64_t)pmax + lown, RCHUNK) * (padded_dh(dh) + 4));
    return s.total();
}

int lvq_attention_extend_shared_lens(const lvq_bf16 *q, const lvq_bf16 *q_lo, const lvq_bf16 *pk_cache, const lvq_bf16 *pk_cache_lo,
                                           const lvq_bf16 *pv_cache, const lvq_bf16 *pv_cache_lo, const lvq_bf16 *k_cache,
                                           const lvq_bf16 *k_cache_lo, const lvq_bf16 *v_cache, const lvq_bf16 *v_cache_lo,
                                           const int32_t *prefix_index, const int32_t *plen, const int32_t *own0, const int32_t *qn,
                                           const int4 *lens, int batch, int lq, int n_heads, int n_kv_heads, int n_prefix, int pmax, int lown, int dh, int64_t q_bstride,
                                           int64_t ldq, int64_t q_hstride, int64_t pk_bstride, int64_t k_bstride, int64_t ldk, int64_t k_hstride,
                                           int64_t pv_bstride, int64_t v_bstride, int64_t ldv, int64_t v_hstride, int64_t o_bstride, int64_t ldo,
                                           int64_t o_hstride, float scale, lvq_bf16 *o, lvq_bf16 *o_lo, void *ws, size_t ws_bytes,
                                           lvq_stream_t stream) {
    const bool x3 = q_lo != nullptr;
    if (!q || !pk_cache || !pv_cache || !k_cache || !v_cache || (!lens && (!prefix_index || !plen || !own0 || !qn)) || !o ||
        !shape_ok(batch, lq, n_heads, n_kv_heads, n_prefix, pmax, lown, dh, x3 ? 3 : 1) || !(scale > 0.f))
        return LVQ_EINVAL;
    // plain, or hi + lo on all five operands
    if (x3 != (pk_cache_lo != nullptr) || x3 != (pv_cache_lo != nullptr) || x3 != (k_cache_lo != nullptr) || x3 != (v_cache_lo != nullptr))
        return LVQ_EINVAL;
    // 16-byte vector loads: every operand row starts on a 16-byte boundary
    for (int64_t s : {q_bstride, ldq, q_hstride, pk_bstride, k_bstride, ldk, k_hstride, pv_bstride, v_bstride, ldv, v_hstride})
        if (s < 0 || s % 8) return LVQ_EINVAL;
    if (o_bstride < 0 || ldo < 0 || o_hstride < 0) return LVQ_EINVAL;
    for (const void *p : {(const void *)q, (const void *)q_lo, (const void *)pk_cache, (const void *)pk_cache_lo, (const void *)pv_cache,
                          (const void *)pv_cache_lo, (const void *)k_cache, (const void *)k_cache_lo, (const void *)v_cache, (const void *)v_cache_lo})
        if (!al16(p)) return LVQ_EINVAL;
    const int dhp = padded_dh(dh);
    LvqArena arena(ws, ws_bytes);
    SharedArgs a;
    a.nchunk = (int)lvq_cdiv((int64_t)pmax + lown, RCHUNK);
    a.ntile = (int)lvq_cdiv((int64_t)lq * (n_heads / n_kv_heads), 16);
    a.part = arena.take<float>((size_t)batch * lq * n_heads * (size_t)a.nchunk * (dhp + 4));
    if (!arena.ok || !al16(a.part)) return LVQ_EWORKSPACE;
    a.q = q; a.ql = q_lo; a.pk = pk_cache; a.pkl = pk_cache_lo; a.pv = pv_cache; a.pvl = pv_cache_lo;
    a.k = k_cache; a.kl = k_cache_lo; a.v = v_cache; a.vl = v_cache_lo;
    a.pidx = prefix_index; a.plen = plen; a.own0 = own0; a.qn = qn; a.lens = lens;
    a.B = batch; a.Lq = lq; a.H = n_heads; a.Hkv = n_kv_heads; a.n_prefix = n_prefix; a.pmax = pmax; a.lown = lown; a.dh = dh;
    a.q_bs = q_bstride; a.ldq = ldq; a.q_hs = q_hstride; a.pk_bs = pk_bstride; a.k_bs = k_bstride; a.ldk = ldk; a.k_hs = k_hstride;
    a.pv_bs = pv_bstride; a.v_bs = v_bstride; a.ldv = ldv; a.v_hs = v_hstride; a.o_bs = o_bstride; a.ldo = ldo; a.o_hs = o_hstride;
    a.scale = scale; a.o = o; a.ol = o_lo;
    hipStream_t st = lvq_s(stream);
    const dim3 grid((unsigned)a.nchunk, (unsigned)(n_kv_heads * a.ntile), (unsigned)batch);
    if (dhp == 64) {
        if (x3) hipLaunchKernelGGL((k_extend_shared<64, 2>), grid, dim3(64), 0, st, a);
        else hipLaunchKernelGGL((k_extend_shared<64, 1>), grid, dim3(64), 0, st, a);
    } else {
        if (x3) hipLaunchKernelGGL((k_extend_shared<128, 2>), grid, dim3(64), 0, st, a);
        else hipLaunchKernelGGL((k_extend_shared<128, 1>), grid, dim3(64), 0, st, a);
    }
    hipLaunchKernelGGL(k_extend_shared_merge, dim3((unsigned)n_heads, (unsigned)lq, (unsigned)batch), dim3(128), 0, st, a, dhp);
    return lvq_launch_status();
}

extern "C" int lvq_attention_extend_shared(const lvq_bf16 *q, const lvq_bf16 *q_lo, const lvq_bf16 *pk_cache, const lvq_bf16 *pk_cache_lo,
                                           const lvq_bf16 *pv_cache, const lvq_bf16 *pv_cache_lo, const lvq_bf16 *k_cache,
                                           const lvq_bf16 *k_cache_lo, const lvq_bf16 *v_cache, const lvq_bf16 *v_cache_lo,
                                           const int32_t *prefix_index, const int32_t *plen, const int32_t *own0, const int32_t *qn, int batch,
                                           int lq, int n_heads, int n_kv_heads, int n_prefix, int pmax, int lown, int dh, int64_t q_bstride,
                                           int64_t ldq, int64_t q_hstride, int64_t pk_bstride, int64_t k_bstride, int64_t ldk, int64_t k_hstride,
                                           int64_t pv_bstride, int64_t v_bstride, int64_t ldv, int64_t v_hstride, int64_t o_bstride, int64_t ldo,
                                           int64_t o_hstride, float scale, lvq_bf16 *o, lvq_bf16 *o_lo, void *ws, size_t ws_bytes,
                                           lvq_stream_t stream) {
    return lvq_attention_extend_shared_lens(q, q_lo, pk_cache, pk_cache_lo, pv_cache, pv_cache_lo, k_cache, k_cache_lo, v_cache, v_cache_lo,
                                            prefix_index, plen, own0, qn, nullptr, batch, lq, n_heads, n_kv_heads, n_prefix, pmax, lown, dh,
                                            q_bstride, ldq, q_hstride, pk_bstride, k_bstride, ldk, k_hstride, pv_bstride, v_bstride, ldv,
                                            v_hstride, o_bstride, ldo, o_hstride, scale, o, o_lo, ws, ws_bytes, stream);
}
