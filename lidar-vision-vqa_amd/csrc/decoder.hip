// csrc/decoder.hip -- one decode step of the Qwen2-architecture stand-in head as ONE native call.
//
// The Python loop of head.StandInHead issues ~14 launches per layer through ctypes at ~9.5 us of host time each: 3.2 ms per token
// for 24 layers although the kernels of a one-token step are microseconds.  This file is the host-side runtime for that loop: the
// same kernels, in the same order, with the same arguments (=> bit-identical logits, tests/test_gpu_head.py), issued from C++.
// inference_engine.py:283-296 -> transformers' generate() with a KV cache is the reference behaviour.
#include "decode_common.h"

namespace {

// rotary embedding at position pos applied in place to the q and k heads of the packed rows (the arithmetic of k_rope in
// elementwise.hip: angle = pos * rope_inv_freq(theta, e, dh), rotate-half pairs), the rotated keys and the values appended to the caches:
// rope + rope + append were three launches of a one-token step
__global__ void __launch_bounds__(256) k_rope_cache(uint16_t *__restrict__ xh, uint16_t *__restrict__ xl, int batch, int n_heads, int n_kv_heads,
                                                    int dh, int pos, int lmax, float theta, uint16_t *__restrict__ kc, uint16_t *__restrict__ kcl,
                                                    uint16_t *__restrict__ vc, uint16_t *__restrict__ vcl) {
    const int per_row = (n_heads + n_kv_heads) * (dh >> 1) + n_kv_heads * dh;   // rotary pairs + value elements to copy
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= batch * per_row) return;
    const int b = i / per_row;
    lvq_rope_cache_item(xh, xl, b, i - b * per_row, n_heads, n_kv_heads, dh, pos, lmax, theta, kc, kcl, vc, vcl);
}

struct StepWs {
    uint16_t *h, *h_lo, *qkv, *qkv_lo, *o, *o_lo, *act, *act_lo;
    float *xb, *gu;
    void *attn;
    size_t attn_bytes;
    int32_t *kv_len;                // ragged step: per-sequence key count of the current token; shared step: four ints per sequence
};
template <typename A> void step_layout(A &a, StepWs &w, int batch, int d, int dkv, int inter, size_t attn_bytes, bool ragged = false, int seqs = 0) {
    const size_t ld = (size_t)d + 2 * dkv;
    w.h = a.template take<uint16_t>((size_t)batch * d);
    w.h_lo = a.template take<uint16_t>((size_t)batch * d);
    w.qkv = a.template take<uint16_t>((size_t)batch * ld);
    w.qkv_lo = a.template take<uint16_t>((size_t)batch * ld);
    w.o = a.template take<uint16_t>((size_t)batch * d);
    w.o_lo = a.template take<uint16_t>((size_t)batch * d);
    w.act = a.template take<uint16_t>((size_t)batch * inter);
    w.act_lo = a.template take<uint16_t>((size_t)batch * inter);
    w.xb = a.template take<float>((size_t)batch * d);
    w.gu = a.template take<float>((size_t)batch * 2 * inter);
    w.attn = a.template take<char>(attn_bytes);
    w.attn_bytes = attn_bytes;
    w.kv_len = ragged ? a.template take<int32_t>(seqs ? (size_t)seqs * 4 : (size_t)batch) : nullptr;
}

// lvq_qwen2_extend_shared: the sequences of the step continue shared prefixes (decode_shared.hip)
struct SharedStep {
    const lvq_qwen2_prefix *prefix;
    const int32_t *prefix_index, *plen, *own0, *qn;
    int batch, lq, n_prefix, pmax;
};

// The layer loop of the entry points.  sh != nullptr: `batch` counts the rows sh->batch * sh->lq, lmax is the length of the own caches and
// the rotary / append launch (which leaves the sequences' clamped lengths in w.kv_len) + lvq_attention_extend_shared stand in place of the ragged pair.
// Otherwise pos0 == nullptr: every sequence at the scalar position `pos` (lvq_qwen2_decode_step: k_rope_cache +
// lvq_attention_bf16 over pos + 1 keys).  pos0 != nullptr: sequence b at pos0[b] + t (lvq_qwen2_decode_step_ragged: the ragged rotary /
// append launch, which also leaves the key counts in w.kv_len, + lvq_attention_decode_ragged).  Everything else is the same calls.
int decode_step(const lvq_qwen2_layer *layers, int n_layers, float *x, int batch, int d, int n_heads, int n_kv_heads, int inter, int pos,
                const int32_t *pos0, int t, int lmax, float rms_eps, float rope_theta, int precision, void *ws, size_t ws_bytes,
                lvq_stream_t stream, const SharedStep *sh = nullptr) {
    const bool ragged = pos0 != nullptr || sh != nullptr;
    const bool x3 = precision == 3;
    const int dh = d / n_heads, dkv = dh * n_kv_heads;
    const int64_t ld = (int64_t)d + 2 * dkv;
    const size_t attn_bytes =
        sh       ? lvq_attention_extend_shared_workspace_bytes(sh->batch, sh->lq, n_heads, n_kv_heads, sh->pmax, lmax, dh, precision)
        : ragged ? lvq_attention_decode_ragged_workspace_bytes(batch, n_heads, n_kv_heads, lmax, dh, precision)
                 : lvq_attention_workspace_bytes(batch, n_heads, 1, lmax, dh, precision);
    if (ragged && attn_bytes == 0) return LVQ_EINVAL;      // a head geometry the ragged attention kernel does not take
    LvqArena arena(ws, ws_bytes);
    StepWs w;
    step_layout(arena, w, batch, d, dkv, inter, attn_bytes, ragged, sh ? sh->batch : 0);
    if (!arena.ok) return LVQ_EWORKSPACE;
    hipStream_t st = lvq_s(stream);
    uint16_t *h_lo = x3 ? w.h_lo : nullptr, *qkv_lo = x3 ? w.qkv_lo : nullptr, *o_lo = x3 ? w.o_lo : nullptr, *act_lo = x3 ? w.act_lo : nullptr;
    const float scale = 1.0f / sqrtf((float)dh);
    float *xa = x, *xb = w.xb;                     // residual stream ping-pong: every layer leaves it in xa again
    int rc;
#define LVQ_TRY(call) do { rc = (call); if (rc != LVQ_OK) return rc; } while (0)
    for (int l = 0; l < n_layers; ++l) {
        const lvq_qwen2_layer &L = layers[l];
        if (x3 && !(L.wqkv_lo && L.wo_lo && L.wgu_lo && L.wdown_lo && L.k_cache_lo && L.v_cache_lo)) return LVQ_EINVAL;
        if (batch <= 8) {                      // RMSNorm fused into the projection (bit-identical to the pair, one launch less)
            LVQ_TRY(lvq_gemv_rmsnorm_bf16(xa, L.ln1, rms_eps, L.wqkv, x3 ? L.wqkv_lo : nullptr, L.bqkv, batch, (int)ld, d, d, ld, nullptr, w.qkv, qkv_lo,
                                          stream));
        } else {
            LVQ_TRY(lvq_rmsnorm(xa, L.ln1, rms_eps, batch, d, nullptr, w.h, h_lo, stream));
            LVQ_TRY(lvq_gemm_bf16(w.h, h_lo, L.wqkv, x3 ? L.wqkv_lo : nullptr, L.bqkv, nullptr, nullptr, 0, 1.0f, 0, batch, (int)ld, d, d, d, ld, 1, 0,
                                  0, 0, nullptr, w.qkv, qkv_lo, stream));
        }
        if (sh) {
            const lvq_qwen2_prefix &P = sh->prefix[l];
            if (!P.k || !P.v || (x3 && !(P.k_lo && P.v_lo))) return LVQ_EINVAL;
            int4 *lens = reinterpret_cast<int4 *>(w.kv_len);         // (g, plen, own, qn) per sequence: layer 0 writes, the rest reads
            lvq_rope_cache_shared(w.qkv, qkv_lo, sh->batch, sh->lq, n_heads, n_kv_heads, dh, sh->prefix_index, sh->plen, sh->n_prefix, sh->pmax,
                                  sh->own0, sh->qn, t, lmax, rope_theta, L.k_cache, x3 ? L.k_cache_lo : nullptr, L.v_cache,
                                  x3 ? L.v_cache_lo : nullptr, l == 0 ? nullptr : lens, lens, st);
            LVQ_TRY(lvq_attention_extend_shared_lens(w.qkv, qkv_lo, P.k, x3 ? P.k_lo : nullptr, P.v, x3 ? P.v_lo : nullptr, L.k_cache,
                                                     x3 ? L.k_cache_lo : nullptr, L.v_cache, x3 ? L.v_cache_lo : nullptr, nullptr, nullptr,
                                                     nullptr, nullptr, lens, sh->batch, sh->lq, n_heads, n_kv_heads, sh->n_prefix, sh->pmax, lmax,
                                                     dh, (int64_t)sh->lq * ld, ld, dh, (int64_t)sh->pmax * dkv, (int64_t)lmax * dkv, dkv, dh,
                                                     (int64_t)sh->pmax * dkv, (int64_t)lmax * dkv, dkv, dh, (int64_t)sh->lq * d, d, dh, scale,
                                                     w.o, o_lo, w.attn, w.attn_bytes, stream));
        } else if (ragged) {
            lvq_rope_cache_ragged(w.qkv, qkv_lo, batch, n_heads, n_kv_heads, dh, pos0, t, lmax, rope_theta, L.k_cache, x3 ? L.k_cache_lo : nullptr,
                                  L.v_cache, x3 ? L.v_cache_lo : nullptr, w.kv_len, st);
            LVQ_TRY(lvq_attention_decode_ragged(w.qkv, qkv_lo, L.k_cache, x3 ? L.k_cache_lo : nullptr, L.v_cache, x3 ? L.v_cache_lo : nullptr, w.kv_len,
                                                batch, n_heads, n_kv_heads, lmax, dh, ld, ld, dh, (int64_t)lmax * dkv, dkv, dh, (int64_t)lmax * dkv, dkv,
                                                dh, d, d, dh, scale, w.o, o_lo, w.attn, w.attn_bytes, stream));
        } else {
            const int per_row = (n_heads + n_kv_heads) * (dh / 2) + dkv;
            hipLaunchKernelGGL(k_rope_cache, dim3((unsigned)lvq_cdiv((int64_t)batch * per_row, 256)), dim3(256), 0, st, w.qkv, qkv_lo, batch, n_heads,
                               n_kv_heads, dh, pos, lmax, rope_theta, L.k_cache, x3 ? L.k_cache_lo : nullptr, L.v_cache,
                               x3 ? L.v_cache_lo : nullptr);
            LVQ_TRY(lvq_attention_bf16(w.qkv, qkv_lo, L.k_cache, x3 ? L.k_cache_lo : nullptr, L.v_cache, x3 ? L.v_cache_lo : nullptr, nullptr, batch,
                                       n_heads, n_kv_heads, 1, pos + 1, dh, ld, ld, dh, (int64_t)lmax * dkv, dkv, dh, (int64_t)lmax * dkv, dkv, dh,
                                       d, d, dh, scale, 0, w.o, o_lo, w.attn, w.attn_bytes, stream));
        }
        LVQ_TRY(lvq_gemm_bf16(w.o, o_lo, L.wo, x3 ? L.wo_lo : nullptr, nullptr, xa, nullptr, 0, 1.0f, 0, batch, d, d, d, d, d, 1, 0, 0, 0, xb,
                              nullptr, nullptr, stream));
        if (batch <= 8) {
            LVQ_TRY(lvq_gemv_rmsnorm_bf16(xb, L.ln2, rms_eps, L.wgu, x3 ? L.wgu_lo : nullptr, nullptr, batch, 2 * inter, d, d, 2 * (int64_t)inter, w.gu,
                                          nullptr, nullptr, stream));
        } else {
            LVQ_TRY(lvq_rmsnorm(xb, L.ln2, rms_eps, batch, d, nullptr, w.h, h_lo, stream));
            LVQ_TRY(lvq_gemm_bf16(w.h, h_lo, L.wgu, x3 ? L.wgu_lo : nullptr, nullptr, nullptr, nullptr, 0, 1.0f, 0, batch, 2 * inter, d, d, d,
                                  2 * (int64_t)inter, 1, 0, 0, 0, w.gu, nullptr, nullptr, stream));
        }
        // (SiLU(gate) * up produced inside the down projection was tried: every one-row wave re-evaluates 4864 exps and IEEE divisions
        //  and reads the fp32 gate|up row -- 16.1 us against 5.3 + 4.9 us for the separate kernels)
        LVQ_TRY(lvq_swiglu(w.gu, batch, inter, w.act, act_lo, stream));
        LVQ_TRY(lvq_gemm_bf16(w.act, act_lo, L.wdown, x3 ? L.wdown_lo : nullptr, nullptr, xb, nullptr, 0, 1.0f, 0, batch, d, inter, inter, inter, d,
                              1, 0, 0, 0, xa, nullptr, nullptr, stream));
    }
#undef LVQ_TRY
    return lvq_launch_status();
}

}  // namespace

extern "C" size_t lvq_qwen2_decode_workspace_bytes(int batch, int d, int n_heads, int n_kv_heads, int inter, int lmax, int precision) {
    if (batch <= 0 || d <= 0 || n_heads <= 0 || n_kv_heads <= 0 || d % n_heads || inter <= 0 || lmax <= 0) return 0;
    const int dh = d / n_heads;
    const size_t attn = lvq_attention_workspace_bytes(batch, n_heads, 1, lmax, dh, precision);
    SizerAdapter a;
    StepWs w;
    step_layout(a, w, batch, d, dh * n_kv_heads, inter, attn);
    return a.s.total();
}

extern "C" int lvq_qwen2_decode_step(const lvq_qwen2_layer *layers, int n_layers, float *x, int batch, int d, int n_heads, int n_kv_heads,
                                     int inter, int pos, int lmax, float rms_eps, float rope_theta, int precision, void *ws, size_t ws_bytes,
                                     lvq_stream_t stream) {
    if (!layers || n_layers <= 0 || !x || batch <= 0 || d <= 0 || n_heads <= 0 || n_kv_heads <= 0 || d % n_heads || n_heads % n_kv_heads ||
        inter <= 0 || pos < 0 || pos >= lmax || (precision != 1 && precision != 3))
        return LVQ_EINVAL;
    return decode_step(layers, n_layers, x, batch, d, n_heads, n_kv_heads, inter, pos, nullptr, 0, lmax, rms_eps, rope_theta, precision, ws, ws_bytes,
                       stream);
}

extern "C" size_t lvq_qwen2_decode_ragged_workspace_bytes(int batch, int d, int n_heads, int n_kv_heads, int inter, int lmax, int precision) {
    if (batch <= 0 || d <= 0 || n_heads <= 0 || n_kv_heads <= 0 || d % n_heads || inter <= 0 || lmax <= 0) return 0;
    const int dh = d / n_heads;
    const size_t attn = lvq_attention_decode_ragged_workspace_bytes(batch, n_heads, n_kv_heads, lmax, dh, precision);
    if (attn == 0) return 0;
    SizerAdapter a;
    StepWs w;
    step_layout(a, w, batch, d, dh * n_kv_heads, inter, attn, true);
    return a.s.total();
}

extern "C" int lvq_qwen2_decode_step_ragged(const lvq_qwen2_layer *layers, int n_layers, float *x, int batch, int d, int n_heads, int n_kv_heads,
                                            int inter, const int32_t *pos0, int t, int lmax, float rms_eps, float rope_theta, int precision,
                                            void *ws, size_t ws_bytes, lvq_stream_t stream) {
    if (!layers || n_layers <= 0 || !x || batch <= 0 || d <= 0 || n_heads <= 0 || n_kv_heads <= 0 || d % n_heads || n_heads % n_kv_heads ||
        inter <= 0 || !pos0 || t < 0 || t >= lmax || (precision != 1 && precision != 3))
        return LVQ_EINVAL;
    return decode_step(layers, n_layers, x, batch, d, n_heads, n_kv_heads, inter, 0, pos0, t, lmax, rms_eps, rope_theta, precision, ws, ws_bytes,
                       stream);
}

extern "C" size_t lvq_qwen2_extend_shared_workspace_bytes(int batch, int lq, int d, int n_heads, int n_kv_heads, int inter, int pmax, int lown,
                                                          int precision) {
    if (batch <= 0 || lq <= 0 || d <= 0 || n_heads <= 0 || n_kv_heads <= 0 || d % n_heads || inter <= 0 || pmax <= 0 || lown <= 0 ||
        (int64_t)batch * lq > (1 << 24))
        return 0;
    const int dh = d / n_heads;
    const size_t attn = lvq_attention_extend_shared_workspace_bytes(batch, lq, n_heads, n_kv_heads, pmax, lown, dh, precision);
    if (attn == 0) return 0;
    SizerAdapter a;
    StepWs w;
    step_layout(a, w, batch * lq, d, dh * n_kv_heads, inter, attn, true, batch);
    return a.s.total();
}

extern "C" int lvq_qwen2_extend_shared(const lvq_qwen2_layer *layers, const lvq_qwen2_prefix *prefix, int n_layers, float *x, int batch, int lq,
                                       int d, int n_heads, int n_kv_heads, int inter, const int32_t *prefix_index, const int32_t *plen,
                                       int n_prefix, int pmax, const int32_t *own0, const int32_t *qn, int t, int lown, float rms_eps,
                                       float rope_theta, int precision, void *ws, size_t ws_bytes, lvq_stream_t stream) {
    if (!layers || !prefix || n_layers <= 0 || !x || batch <= 0 || lq <= 0 || (int64_t)batch * lq > (1 << 24) || d <= 0 || n_heads <= 0 ||
        n_kv_heads <= 0 || d % n_heads || n_heads % n_kv_heads || inter <= 0 || !prefix_index || !plen || n_prefix <= 0 || pmax <= 0 || !own0 ||
        !qn || t < 0 || t >= lown || (precision != 1 && precision != 3))
        return LVQ_EINVAL;
    const SharedStep sh = {prefix, prefix_index, plen, own0, qn, batch, lq, n_prefix, pmax};
    return decode_step(layers, n_layers, x, batch * lq, d, n_heads, n_kv_heads, inter, 0, nullptr, t, lown, rms_eps, rope_theta, precision, ws,
                       ws_bytes, stream, &sh);
}
