// csrc/decode_common.h -- pieces shared by the scalar-position decode step (decoder.hip), the ragged one (decode_ragged.hip) and the
// shared-prefix one (decode_shared.hip)
#pragma once
#include "common.h"

// Keys per attention work unit of decode_ragged.hip and decode_shared.hip: FIXED, so that a sequence's work units depend on its own
// lengths only, and equal in both files, so that one query row over equal keys has the same keys in the same lanes in both.
constexpr int LVQ_RCHUNK = 128;
constexpr int LVQ_RKVB = 64;            // keys per MFMA tile of those kernels
static_assert(LVQ_RCHUNK % LVQ_RKVB == 0, "a chunk is whole key tiles");

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

// two fp32 -> packed bf16 pair (v_cvt_pk_bf16_f32: round-to-nearest-even)
__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
    bf16x2_t p = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(uint32_t, p);
}
// max over the four lane groups g = lane >> 4 that hold different keys of the same query
__device__ __forceinline__ float max_over_groups(float x) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

// Work item j of sequence b of the rotary + cache-append pass of a one-token decode step: rotary embedding at position pos applied in
// place to the q and k heads of the packed q|k|v row (the arithmetic of k_rope in elementwise.hip: angle = pos * rope_inv_freq(theta,
// e, dh), rotate-half pairs), the rotated keys and the values appended to the caches at row pos.  j < (n_heads + n_kv_heads) * dh / 2:
// a rotary pair; above: one value element.  One body for all kernels, so equal positions give equal bits.
// The general form: the packed row is `row`, the rotary position `pos`, and the cache row that takes the key / value is `crow` (counted
// over the whole cache buffer: sequence * rows per sequence + row), so the rotary position and the cache row may differ.
__device__ __forceinline__ void lvq_rope_cache_item_at(uint16_t *__restrict__ xh, uint16_t *__restrict__ xl, int64_t row, int j, int n_heads,
                                                       int n_kv_heads, int dh, int pos, int64_t crow, float theta, uint16_t *__restrict__ kc,
                                                       uint16_t *__restrict__ kcl, uint16_t *__restrict__ vc, uint16_t *__restrict__ vcl) {
    const int half = dh >> 1, d = n_heads * dh, dkv = n_kv_heads * dh;
    const int64_t ld = d + 2 * dkv;
    const int nrope = (n_heads + n_kv_heads) * half;           // rotary pairs per row
    if (j < nrope) {
        const int hd = j / half, e = j - hd * half;
        const float inv = rope_inv_freq(theta, e, dh);
        float sn, cs;
        sincosf((float)pos * inv, &sn, &cs);
        const int64_t o1 = row * ld + (int64_t)hd * dh + e, o2 = o1 + half;
        const float a = bf16_to_f32(xh[o1]) + (xl ? bf16_to_f32(xl[o1]) : 0.f);
        const float bb = bf16_to_f32(xh[o2]) + (xl ? bf16_to_f32(xl[o2]) : 0.f);
        const float ra = a * cs - bb * sn, rb = bb * cs + a * sn;
        const uint16_t ha = f32_to_bf16(ra), hb = f32_to_bf16(rb);
        xh[o1] = ha; xh[o2] = hb;
        uint16_t la = 0, lb = 0;
        if (xl) { la = f32_to_bf16(ra - bf16_to_f32(ha)); lb = f32_to_bf16(rb - bf16_to_f32(hb)); xl[o1] = la; xl[o2] = lb; }
        if (hd >= n_heads) {                                   // a key head: the rotated pair also goes to the cache
            const int c = (hd - n_heads) * dh + e;
            const int64_t dst = crow * dkv + c;
            kc[dst] = ha; kc[dst + half] = hb;
            if (xl) { kcl[dst] = la; kcl[dst + half] = lb; }
        }
    } else {
        const int c = j - nrope;
        const int64_t src = row * ld + d + dkv + c, dst = crow * dkv + c;
        vc[dst] = xh[src];
        if (xl) vcl[dst] = xl[src];
    }
}
// a one-token step: the packed row of sequence b at position pos goes to row pos of that sequence's cache [lmax rows]
__device__ __forceinline__ void lvq_rope_cache_item(uint16_t *__restrict__ xh, uint16_t *__restrict__ xl, int b, int j, int n_heads, int n_kv_heads,
                                                    int dh, int pos, int lmax, float theta, uint16_t *__restrict__ kc, uint16_t *__restrict__ kcl,
                                                    uint16_t *__restrict__ vc, uint16_t *__restrict__ vcl) {
    lvq_rope_cache_item_at(xh, xl, b, j, n_heads, n_kv_heads, dh, pos, (int64_t)b * lmax + pos, theta, kc, kcl, vc, vcl);
}

// decode_ragged.hip: the rotary + cache-append launch of lvq_qwen2_decode_step_ragged.  Sequence b works at position
// min(max(pos0[b] + t, 0), lmax - 1) and its key count (that position + 1) is written to kv_len[b] for the attention call behind it.
void lvq_rope_cache_ragged(uint16_t *xh, uint16_t *xl, int batch, int n_heads, int n_kv_heads, int dh, const int32_t *pos0, int t, int lmax,
                           float theta, uint16_t *kc, uint16_t *kcl, uint16_t *vc, uint16_t *vcl, int32_t *kv_len, hipStream_t st);

// decode_shared.hip: the rotary + cache-append launch of lvq_qwen2_extend_shared.  Query row r < qn[b] of sequence b (packed row b * lq + r)
// is rotated at position plen[prefix_index[b]] + own and appended to row own = min(own0[b] + t + r, lown - 1) of the sequence's own cache.
// lens_in == nullptr: the lengths come from the four arrays and (g, plen[g], own0[b] + t, qn[b]), clamped, are left in lens_out[b];
// lens_in != nullptr: they are read from there.  The record is the same for every layer of a step, so the first layer writes it and
// every later launch of the step -- rotary, attention, merge -- reads it with ONE load instead of the dependent pair
// prefix_index[b] -> plen[g]: that chain was what made the one-row shared step measurably slower than the ragged step.
void lvq_rope_cache_shared(uint16_t *xh, uint16_t *xl, int batch, int lq, int n_heads, int n_kv_heads, int dh, const int32_t *prefix_index,
                           const int32_t *plen, int n_prefix, int pmax, const int32_t *own0, const int32_t *qn, int t, int lown, float theta,
                           uint16_t *kc, uint16_t *kcl, uint16_t *vc, uint16_t *vcl, const int4 *lens_in, int4 *lens_out, hipStream_t st);
// lvq_attention_extend_shared with the per-sequence records of lvq_rope_cache_shared (lens != nullptr: the four arrays are unused)
int lvq_attention_extend_shared_lens(const lvq_bf16 *q, const lvq_bf16 *q_lo, const lvq_bf16 *pk_cache, const lvq_bf16 *pk_cache_lo,
                                     const lvq_bf16 *pv_cache, const lvq_bf16 *pv_cache_lo, const lvq_bf16 *k_cache, const lvq_bf16 *k_cache_lo,
                                     const lvq_bf16 *v_cache, const lvq_bf16 *v_cache_lo, const int32_t *prefix_index, const int32_t *plen,
                                     const int32_t *own0, const int32_t *qn, const int4 *lens, int batch, int lq, int n_heads, int n_kv_heads,
                                     int n_prefix, int pmax, int lown, int dh, int64_t q_bstride, int64_t ldq, int64_t q_hstride,
                                     int64_t pk_bstride, int64_t k_bstride, int64_t ldk, int64_t k_hstride, int64_t pv_bstride, int64_t v_bstride,
                                     int64_t ldv, int64_t v_hstride, int64_t o_bstride, int64_t ldo, int64_t o_hstride, float scale, lvq_bf16 *o,
                                     lvq_bf16 *o_lo, void *ws, size_t ws_bytes, lvq_stream_t stream);
