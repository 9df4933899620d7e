// csrc/decode_common.h -- pieces shared by the scalar-position decode step (decoder.hip) and the ragged one (decode_ragged.hip)
#pragma once
#include "common.h"

// Work item j of sequence b of the rotary + cache-append pass of a one-token decode step: rotary embedding at position pos applied in
// place to the q and k heads of the packed q|k|v row (the arithmetic of k_rope in elementwise.hip: angle = pos * rope_inv_freq(theta,
// e, dh), rotate-half pairs), the rotated keys and the values appended to the caches at row pos.  j < (n_heads + n_kv_heads) * dh / 2:
// a rotary pair; above: one value element.  One body for both kernels, so equal positions give equal bits.
__device__ __forceinline__ void lvq_rope_cache_item(uint16_t *__restrict__ xh, uint16_t *__restrict__ xl, int b, int j, int n_heads, int n_kv_heads,
                                                    int dh, int pos, int lmax, float theta, uint16_t *__restrict__ kc, uint16_t *__restrict__ kcl,
                                                    uint16_t *__restrict__ vc, uint16_t *__restrict__ vcl) {
    const int half = dh >> 1, d = n_heads * dh, dkv = n_kv_heads * dh;
    const int64_t ld = d + 2 * dkv;
    const int nrope = (n_heads + n_kv_heads) * half;           // rotary pairs per row
    if (j < nrope) {
        const int hd = j / half, e = j - hd * half;
        const float inv = rope_inv_freq(theta, e, dh);
        float sn, cs;
        sincosf((float)pos * inv, &sn, &cs);
        const int64_t o1 = (int64_t)b * ld + (int64_t)hd * dh + e, o2 = o1 + half;
        const float a = bf16_to_f32(xh[o1]) + (xl ? bf16_to_f32(xl[o1]) : 0.f);
        const float bb = bf16_to_f32(xh[o2]) + (xl ? bf16_to_f32(xl[o2]) : 0.f);
        const float ra = a * cs - bb * sn, rb = bb * cs + a * sn;
        const uint16_t ha = f32_to_bf16(ra), hb = f32_to_bf16(rb);
        xh[o1] = ha; xh[o2] = hb;
        uint16_t la = 0, lb = 0;
        if (xl) { la = f32_to_bf16(ra - bf16_to_f32(ha)); lb = f32_to_bf16(rb - bf16_to_f32(hb)); xl[o1] = la; xl[o2] = lb; }
        if (hd >= n_heads) {                                   // a key head: the rotated pair also goes to the cache
            const int c = (hd - n_heads) * dh + e;
            const int64_t dst = ((int64_t)b * lmax + pos) * dkv + c;
            kc[dst] = ha; kc[dst + half] = hb;
            if (xl) { kcl[dst] = la; kcl[dst + half] = lb; }
        }
    } else {
        const int c = j - nrope;
        const int64_t src = (int64_t)b * ld + d + dkv + c, dst = ((int64_t)b * lmax + pos) * dkv + c;
        vc[dst] = xh[src];
        if (xl) vcl[dst] = xl[src];
    }
}

// decode_ragged.hip: the rotary + cache-append launch of lvq_qwen2_decode_step_ragged.  Sequence b works at position
// min(max(pos0[b] + t, 0), lmax - 1) and its key count (that position + 1) is written to kv_len[b] for the attention call behind it.
void lvq_rope_cache_ragged(uint16_t *xh, uint16_t *xl, int batch, int n_heads, int n_kv_heads, int dh, const int32_t *pos0, int t, int lmax,
                           float theta, uint16_t *kc, uint16_t *kcl, uint16_t *vc, uint16_t *vcl, int32_t *kv_len, hipStream_t st);
