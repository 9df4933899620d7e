// csrc/clip_embed.hip -- the embedding step of the CLIP-L tower on channel-major patch features (include/lvq.h: lvq_clip_embed)
//
//   hidden[b (1 + hw) + 0    , :] = LayerNorm(cls          + pos[0    , :])                (clip_sdpa.py:160-167, 363)
//   hidden[b (1 + hw) + 1 + p, :] = LayerNorm(feat[b, :, p] + pos[1 + p, :])
//   tok   [b hw + p, 0 .. c)      = bf16 (hi, lo) of feat[b, :, p]                           (the projector's SAM operand)
//
// As torch copies this is flatten + transpose, cat with the class row, the position add and the norm -- four passes over the
// activation -- and a second permute of the same features for the projector.  Here one workgroup owns a tile of TT = 16 consecutive
// tokens of the flat [batch * hw] token axis (a tile may straddle images) and all c channels:
//   1. read   lane = (token tid & 15, channel tid >> 4): 16 consecutive floats of one channel row = 64 contiguous bytes per 16 lanes
//   2. LDS    tile[token][channel] with a row of c + 2 floats.  ds_write_b32 banks are (dword address) % 32 within 32 lanes: a write
//             covers tokens 0..15 x two channels, address token (c + 2) + channel == 2 token + channel (mod 32, c % 64 == 0): 32 distinct
//             banks.  The row read is ds_read_b64 at 2 lane + 128 j: 64 consecutive dwords per 32 lanes, one per bank of the 64.
//   3. write  wave w takes tokens 4 w .. 4 w + 3, one row at a time, lanes along c (8 bytes each: 512-byte stores of `hidden`, 256-byte
//             stores of the bf16 rows); the row lives in registers (<= 32 floats per lane) between the two statistics passes.
// The class row has no source in `feat`: the wave that owns token p = 0 of image b also writes row b (1 + hw) from `cls`.
// LDS: 16 (c + 2) 4 bytes = 64.1 KiB at c = 1024 (two workgroups = 8 waves per CU), 128.1 KiB at c = 2048 (one).
#include "common.h"

namespace {

constexpr int TT = 16;           // tokens per workgroup
constexpr int MAXJ = 16;         // 128-channel steps of a row: c <= 2048

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one row by one wave: x (LDS token row or the class embedding) + pos row -> LayerNorm -> hidden row
template <bool FROM_LDS>
__device__ __forceinline__ void embed_row(const float *__restrict__ src, const float *__restrict__ posr, const float *__restrict__ gamma,
                                          const float *__restrict__ beta, float eps, int c, int lane, float *__restrict__ out) {
    float2 r[MAXJ];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const int k = 2 * lane + 128 * j;
        r[j] = make_float2(0.f, 0.f);
        if (k < c) {
            const float2 x = *reinterpret_cast<const float2 *>(src + k), p = *reinterpret_cast<const float2 *>(posr + k);
            r[j] = make_float2(x.x + p.x, x.y + p.y);
        }
        s += r[j].x + r[j].y;                                  // padding slots hold 0
    }
    const float mean = wave_sum(s) / (float)c;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        if (2 * lane + 128 * j < c) {
            r[j].x -= mean; r[j].y -= mean;
            q += r[j].x * r[j].x + r[j].y * r[j].y;
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)c + eps);
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
        const int k = 2 * lane + 128 * j;
        if (k < c) {
            const float2 g = *reinterpret_cast<const float2 *>(gamma + k);
            float2 y = make_float2(r[j].x * rstd * g.x, r[j].y * rstd * g.y);
            if (beta) { const float2 b = *reinterpret_cast<const float2 *>(beta + k); y.x += b.x; y.y += b.y; }
            *reinterpret_cast<float2 *>(out + k) = y;
        }
    }
}

__global__ void __launch_bounds__(256) k_clip_embed(const float *__restrict__ feat, const float *__restrict__ cls, const float *__restrict__ pos,
                                                    const float *__restrict__ gamma, const float *__restrict__ beta, float eps, int64_t ntok,
                                                    int c, int hw, float *__restrict__ hidden, uint16_t *__restrict__ tok_hi,
                                                    uint16_t *__restrict__ tok_lo, int64_t ld_tok) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int ld = c + 2;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * TT;
    {
        const int tl = tid & 15;
        const int64_t t = t0 + tl;
        if (t < ntok) {
            const int64_t b = t / hw;
            const int p = (int)(t - b * hw);
            const float *src = feat + (b * c) * hw + p;
#pragma unroll 4
            for (int ch = tid >> 4; ch < c; ch += 16) tile[tl * ld + ch] = src[(int64_t)ch * hw];
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < TT / 4; ++i) {
        const int tl = wid * (TT / 4) + i;
        const int64_t t = t0 + tl;
        if (t >= ntok) break;                                   // wave-uniform
        const int64_t b = t / hw;
        const int p = (int)(t - b * hw);
        const float *row = tile + tl * ld;
        const int64_t hrow = b * (1 + (int64_t)hw) + 1 + p;
        embed_row<true>(row, pos + (int64_t)(1 + p) * c, gamma, beta, eps, c, lane, hidden + hrow * c);
        if (p == 0) embed_row<false>(cls, pos, gamma, beta, eps, c, lane, hidden + (hrow - 1) * c);
        if (tok_hi) {
            // lvq_cast_bf16's expressions on the untouched feature values
#pragma unroll
            for (int j = 0; j < MAXJ; ++j) {
                const int k = 2 * lane + 128 * j;
                if (k < c) {
                    const float2 x = *reinterpret_cast<const float2 *>(row + k);
                    const uint16_t h0 = f32_to_bf16(x.x), h1 = f32_to_bf16(x.y);
                    *reinterpret_cast<uint32_t *>(tok_hi + t * ld_tok + k) = (uint32_t)h0 | ((uint32_t)h1 << 16);
                    if (tok_lo)
                        *reinterpret_cast<uint32_t *>(tok_lo + t * ld_tok + k) =
                            (uint32_t)f32_to_bf16(x.x - bf16_to_f32(h0)) | ((uint32_t)f32_to_bf16(x.y - bf16_to_f32(h1)) << 16);
                }
            }
        }
    }
}

}  // namespace

extern "C" int lvq_clip_embed_ok(int batch, int c, int hw) { return batch >= 1 && hw >= 1 && c >= 64 && c <= 2048 && c % 64 == 0; }

extern "C" int lvq_clip_embed(const float *feat, const float *cls, const float *pos, const float *gamma, const float *beta, float eps,
                              int batch, int c, int hw, float *hidden, lvq_bf16 *tok_hi, lvq_bf16 *tok_lo, int64_t ld_tok,
                              lvq_stream_t stream) {
    if (batch <= 0 || c <= 0 || hw <= 0 || !feat || !cls || !pos || !gamma || !hidden || (tok_lo && !tok_hi)) return LVQ_EINVAL;
    if (!lvq_clip_embed_ok(batch, c, hw)) return LVQ_EUNSUPPORTED;
    if ((int64_t)batch * (1 + (int64_t)hw) > 0x7fffffff) return LVQ_EUNSUPPORTED;
    if (((uintptr_t)feat | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)hidden) & 15) return LVQ_EUNSUPPORTED;
    if (tok_hi && ((((uintptr_t)tok_hi | (uintptr_t)tok_lo) & 3) || (ld_tok & 1) || ld_tok < c)) return LVQ_EUNSUPPORTED;
    const size_t lds = (size_t)TT * (c + 2) * sizeof(float);
    static LvqLdsOnce once;
    if (lds > 64 * 1024 && !lvq_ensure_lds(once, {(const void *)k_clip_embed}, 160 * 1024)) return LVQ_ELAUNCH;
    const int64_t ntok = (int64_t)batch * hw;
    hipLaunchKernelGGL(k_clip_embed, dim3((unsigned)lvq_cdiv(ntok, TT)), dim3(256), lds, lvq_s(stream), feat, cls, pos, gamma, beta, eps, ntok, c,
                       hw, hidden, tok_hi, tok_lo, ld_tok);
    return lvq_launch_status();
}
