// csrc/conv2d.hip -- the dense 2-D convolutions of BaseBEVBackbone (pcdet/models/backbones_2d/base_bev_backbone.py:6-204: 3 x 3 conv + eval
// BatchNorm + ReLU stacks at stride 1 / 2, ConvTranspose2d(kernel = stride) or strided-conv deblocks, channel concat), gfx950.
//
//   lvq_conv2d_to_planes     [B, C, H, W] fp32 -> channels-last operand planes [B, H, W, Cp] bf16 hi (+ lo), Cp = C rounded up to 32, zeros beyond C.
//                            Activations stay in this form between layers: a conv's epilogue writes the next conv's operand.
//   lvq_conv2d_pack_weights  torch's [C_out, C_in, k, k] (conv) or [C_in, C_out, s, s] (transposed conv) fp32 -> MFMA-fragment order
//                            [Cp / 32][tap][N / 16][lane 64][8] bf16 hi (+ lo): the B fragment of a wave is one contiguous 1 KiB read.
//   lvq_conv2d / lvq_deconv2d  implicit GEMM on v_mfma_f32_16x16x32_bf16, fp32 accumulators.  One workgroup = an 8 x 8 tile of output pixels
//                            x 64 output columns of one scene; its four waves are 2 x 2 (32 pixels x 32 columns each).  Per channel chunk the
//                            input tile WITH ITS HALO ((7 s + 3)^2 pixels for kernel 3) is staged in LDS once, cells outside the canvas as
//                            zeros, and each of the nine taps reads its shifted window out of that one tile: no neighbour table, no gather,
//                            no border branch in the MFMA loop.  kernel = stride has no halo and no reuse: each tap stages its own 8 x 8
//                            pixels.  The transposed conv is the 1 x 1 case with N = s^2 C_out columns and a pixel-shuffle epilogue.
//                            Epilogue [relu](acc * scale + shift) from the accumulators into operand planes and / or fp32 [B, C, H, W], both
//                            with a channel offset inside a wider buffer (the concat is never a copy).
//   lvq_conv2d_res           the same kernel body with residual planes [B, OH, OW, c_out] in the epilogue, [relu](acc * scale + shift + res):
//                            the dense BasicBlock of PillarRes18BackBone8x (spconv_backbone_2d.py:79-111).  Its own argument record, so the
//                            arguments and registers of the plain instantiations do not move.
//   order                    channel chunks ascending, taps ascending inside a chunk, 32-channel steps ascending inside a tap, hi*hi + hi*lo +
//                            lo*hi; no atomics.  A pixel's bits depend on its receptive field only.
#include "common.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

namespace {

constexpr int TH = 8, TW = 8, BN = 64;
constexpr int MAXC = 512;

int pad32(int c) { return (c + 31) / 32 * 32; }
// the family, stated once (include/lvq.h repeats it): c_in 1 .. 512 (planes hold c_in rounded up to 32), c_out a multiple of 64 in 64 .. 512
bool cin_ok(int c) { return c >= 1 && c <= MAXC; }
bool cout_ok(int c) { return c >= BN && c <= MAXC && c % BN == 0; }
// (kernel, stride): 3 with padding 1 at stride 1 / 2; kernel = stride in {1, 2, 4} with padding 0
bool geom_ok(int k, int s) { return (k == 3 && (s == 1 || s == 2)) || (k == s && (s == 1 || s == 2 || s == 4)); }

struct ConvArgs {
    const uint16_t *in_hi, *in_lo;
    const uint16_t *w_hi, *w_lo;
    const float *scale, *shift;
    uint16_t *out_hi, *out_lo;
    float *out_f32;
    int h, w, cp;                 // input canvas, channels of the input planes
    int oh, ow;                   // conv output (before the pixel shuffle)
    int n_total, c_out, ups;      // GEMM columns = ups^2 * c_out
    int c_total, c_off, relu;
    int tiles_x;
    static constexpr bool RES = false;
};
struct ConvResArgs : ConvArgs {
    const uint16_t *res_hi, *res_lo;              // [B, OH, OW, c_out]; res_lo may be NULL
    static constexpr bool RES = true;
};

__global__ void __launch_bounds__(256) k_to_planes(const float *__restrict__ x, int c, int64_t hw, int cp, uint16_t *__restrict__ hi,
                                                   uint16_t *__restrict__ lo) {
    __shared__ float s[32][65];
    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int c0 = blockIdx.y * 32, b = blockIdx.z;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int cc = i * 4 + (tid >> 6), px = tid & 63;
        s[cc][px] = (c0 + cc < c && p0 + px < hw) ? x[((int64_t)b * c + c0 + cc) * hw + p0 + px] : 0.f;
    }
    __syncthreads();
    const int px = tid >> 2, g = (tid & 3) * 8;
    if (p0 + px >= hw) return;
    uint32_t h[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float v0 = s[g + 2 * j][px], v1 = s[g + 2 * j + 1][px];
        const uint16_t h0 = f32_to_bf16(v0), h1 = f32_to_bf16(v1);
        h[j] = (uint32_t)h0 | ((uint32_t)h1 << 16);
        l[j] = (uint32_t)f32_to_bf16(v0 - bf16_to_f32(h0)) | ((uint32_t)f32_to_bf16(v1 - bf16_to_f32(h1)) << 16);
    }
    const int64_t o = ((int64_t)b * hw + p0 + px) * cp + c0 + g;
    *reinterpret_cast<uint4 *>(hi + o) = make_uint4(h[0], h[1], h[2], h[3]);
    if (lo) *reinterpret_cast<uint4 *>(lo + o) = make_uint4(l[0], l[1], l[2], l[3]);
}

// element t of the packed weights: [cp / 32][taps][n_total / 16][lane][8]; lane = 16 (k / 8) + column, as the MFMA B operand wants it
__global__ void __launch_bounds__(256) k_pack_w2d(const float *__restrict__ w, int c_out, int c_in, int k, int transposed, int64_t total,
                                                  uint16_t *__restrict__ hi, uint16_t *__restrict__ lo) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int taps = transposed ? 1 : k * k, n_total = transposed ? c_out * k * k : c_out;
    const int e = (int)(t & 7), lane = (int)((t >> 3) & 63);
    int64_t rest = t >> 9;
    const int nt = (int)(rest % (n_total / 16));
    rest /= n_total / 16;
    const int tap = (int)(rest % taps), kidx = (int)(rest / taps);
    const int n = nt * 16 + (lane & 15), ci = kidx * 32 + (lane >> 4) * 8 + e;
    float v = 0.f;
    if (ci < c_in) {
        if (transposed) {
            const int co = n % c_out, sub = n / c_out;                  // sub = i * s + j: weight [c_in, c_out, s, s]
            v = w[((int64_t)ci * c_out + co) * k * k + sub];
        } else {
            v = w[((int64_t)n * c_in + ci) * k * k + tap];              // weight [c_out, c_in, k, k], tap = ky * k + kx
        }
    }
    const uint16_t h = f32_to_bf16(v);
    hi[t] = h;
    if (lo) lo[t] = f32_to_bf16(v - bf16_to_f32(h));
}

// A = ConvArgs, or ConvResArgs: the residual planes [B, OH, OW, c_out] join the epilogue (ups = 1 only).  The residual form has an argument
// record of its own, so ConvArgs -- and with it every register of the plain instantiations -- stays as it is.
template <int K, int S, int CK, bool SPLIT, typename A = ConvArgs>
__global__ void __launch_bounds__(256) k_conv2d(const A a) {
    constexpr bool HALO = K == 3;
    constexpr int TAPS = K * K, KS = CK / 32, PITCH = CK + 8;           // bf16 elements; rows stay 16-byte aligned
    constexpr int RH = HALO ? (TH - 1) * S + K : TH, RW = HALO ? (TW - 1) * S + K : TW;      // the staged region, in pixels
    constexpr int RSTEP = HALO ? 1 : S, AS = HALO ? S : 1;              // canvas step between staged pixels; LDS step between output pixels
    constexpr int PHASES = HALO ? 1 : TAPS, TPP = HALO ? TAPS : 1;      // stagings per channel chunk, taps per staging
    constexpr int QPP = CK / 8;                                         // 16-byte pieces per pixel
    __shared__ __attribute__((aligned(16))) uint16_t s_hi[RH * RW * PITCH];
    __shared__ __attribute__((aligned(16))) uint16_t s_lo[SPLIT ? RH * RW * PITCH : 8];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int wm = wid >> 1, wn = wid & 1;
    const int oy0 = ((int)blockIdx.x / a.tiles_x) * TH, ox0 = ((int)blockIdx.x % a.tiles_x) * TW;
    const int nblk = blockIdx.y, b = blockIdx.z;
    const int nt16 = a.n_total / 16;
    const int64_t in_base = (int64_t)b * a.h * a.w;

    f32x4 acc[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // LDS pixel of this lane's A rows (tile pixel p = 16 (2 wm + mt) + l15 -> row p / 8, column p % 8)
    int arow[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int p = wm * 32 + mt * 16 + l15;
        arow[mt] = ((p >> 3) * AS * RW + (p & 7) * AS) * PITCH + 8 * lq;
    }
    const int ntile0 = nblk * (BN / 16) + wn * 2;

    for (int c0 = 0; c0 < a.cp; c0 += CK) {
        for (int ph = 0; ph < PHASES; ++ph) {
            const int gy0 = oy0 * S + (HALO ? -1 : ph / K), gx0 = ox0 * S + (HALO ? -1 : ph % K);
            __syncthreads();                                            // the previous staging has been read
            for (int e = tid; e < RH * RW * QPP; e += 256) {
                const int pix = e / QPP, part = e % QPP;
                const int iy = gy0 + (pix / RW) * RSTEP, ix = gx0 + (pix % RW) * RSTEP;
                uint4 vh = make_uint4(0u, 0u, 0u, 0u), vl = vh;         // outside the canvas: zeros, so a border pixel runs the interior's code
                if (iy >= 0 && iy < a.h && ix >= 0 && ix < a.w) {
                    const int64_t g = (in_base + (int64_t)iy * a.w + ix) * a.cp + c0 + part * 8;
                    vh = *reinterpret_cast<const uint4 *>(a.in_hi + g);
                    if (SPLIT) vl = *reinterpret_cast<const uint4 *>(a.in_lo + g);
                }
                *reinterpret_cast<uint4 *>(&s_hi[pix * PITCH + part * 8]) = vh;
                if (SPLIT) *reinterpret_cast<uint4 *>(&s_lo[pix * PITCH + part * 8]) = vl;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < TPP; ++t) {
                const int tap = HALO ? t : ph;
                const int aoff = HALO ? ((t / K) * RW + (t % K)) * PITCH : 0;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const int64_t wofs = ((((int64_t)(c0 / 32 + ks) * TAPS + tap) * nt16 + ntile0) * 64 + lane) * 8;
                    bf16x8 bh[2], bl[2], ah[2], al[2];
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        bh[nt] = *reinterpret_cast<const bf16x8 *>(a.w_hi + wofs + nt * 512);
                        bl[nt] = SPLIT ? *reinterpret_cast<const bf16x8 *>(a.w_lo + wofs + nt * 512) : bh[nt];
                    }
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        ah[mt] = *reinterpret_cast<const bf16x8 *>(&s_hi[arow[mt] + aoff + ks * 32]);
                        al[mt] = SPLIT ? *reinterpret_cast<const bf16x8 *>(&s_lo[arow[mt] + aoff + ks * 32]) : ah[mt];
                    }
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt) {
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], bh[nt], acc[mt][nt], 0, 0, 0);
                            if (SPLIT) {
                                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], bl[nt], acc[mt][nt], 0, 0, 0);
                                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[mt], bh[nt], acc[mt][nt], 0, 0, 0);
                            }
                        }
                }
            }
        }
    }
    // epilogue: accumulator element j of lane l is (row 4 (l >> 4) + j, column l & 15) of a 16 x 16 tile
    const int ohs = a.oh * a.ups, ows = a.ow * a.ups;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int n = (ntile0 + nt) * 16 + l15;
        const int co = n % a.c_out, sub = n / a.c_out;
        const int si = sub / a.ups, sj = sub % a.ups;
        const float sc = a.scale ? a.scale[co] : 1.f, sh = a.scale ? a.shift[co] : 0.f;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int p = wm * 32 + mt * 16 + lq * 4 + j;
                const int oy = oy0 + (p >> 3), ox = ox0 + (p & 7);
                if (oy >= a.oh || ox >= a.ow) continue;
                float v = acc[mt][nt][j];
                if (a.scale) v = v * sc + sh;
                if constexpr (A::RES) {
                    const int64_t r = (((int64_t)b * a.oh + oy) * a.ow + ox) * a.c_out + co;
                    float res = bf16_to_f32(a.res_hi[r]);
                    if (a.res_lo) res += bf16_to_f32(a.res_lo[r]);
                    v += res;
                }
                if (a.relu) v = v > 0.f ? v : 0.f;
                const int y = oy * a.ups + si, x = ox * a.ups + sj;
                if (a.out_hi) {
                    const int64_t o = (((int64_t)b * ohs + y) * ows + x) * a.c_total + a.c_off + co;
                    const uint16_t h = f32_to_bf16(v);
                    a.out_hi[o] = h;
                    if (a.out_lo) a.out_lo[o] = f32_to_bf16(v - bf16_to_f32(h));
                }
                if (a.out_f32) a.out_f32[(((int64_t)b * a.c_total + a.c_off + co) * ohs + y) * ows + x] = v;
            }
        }
    }
}

template <int K, int S, int CK>
void launch_split(bool split, dim3 grid, hipStream_t st, const ConvArgs &a, const lvq_bf16 *res_hi, const lvq_bf16 *res_lo) {
    if (res_hi) {
        ConvResArgs ra;
        static_cast<ConvArgs &>(ra) = a;
        ra.res_hi = res_hi; ra.res_lo = res_lo;
        if (split)
            hipLaunchKernelGGL((k_conv2d<K, S, CK, true, ConvResArgs>), grid, dim3(256), 0, st, ra);
        else
            hipLaunchKernelGGL((k_conv2d<K, S, CK, false, ConvResArgs>), grid, dim3(256), 0, st, ra);
    } else if (split)
        hipLaunchKernelGGL((k_conv2d<K, S, CK, true>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((k_conv2d<K, S, CK, false>), grid, dim3(256), 0, st, a);
}

// the shared body of lvq_conv2d, lvq_conv2d_res (ups = 1; res_hi != NULL) and lvq_deconv2d (kernel = stride = 1 on the canvas, ups = s)
int run_conv(const lvq_bf16 *in_hi, const lvq_bf16 *in_lo, int batch, int h, int w, int c_in, const lvq_bf16 *w_hi, const lvq_bf16 *w_lo, int c_out,
             int kernel, int stride, int ups, const float *scale, const float *shift, int relu, lvq_bf16 *out_hi, lvq_bf16 *out_lo, float *out_f32,
             int out_c_total, int out_c_off, lvq_stream_t stream, const lvq_bf16 *res_hi = nullptr, const lvq_bf16 *res_lo = nullptr) {
    if (batch <= 0 || h <= 0 || w <= 0 || c_in <= 0 || c_out <= 0 || kernel <= 0 || stride <= 0) return LVQ_EINVAL;
    if ((scale == nullptr) != (shift == nullptr) || (in_lo == nullptr) != (w_lo == nullptr)) return LVQ_EINVAL;
    if (!in_hi || !w_hi || (!out_hi && !out_f32) || (out_lo && !out_hi)) return LVQ_EINVAL;
    if (out_c_off < 0 || out_c_total <= 0 || (int64_t)out_c_off + c_out > out_c_total) return LVQ_EINVAL;
    if (!cin_ok(c_in) || !cout_ok(c_out) || !geom_ok(kernel, stride) || batch > 65535) return LVQ_EUNSUPPORTED;
    if (((uintptr_t)in_hi | (uintptr_t)in_lo | (uintptr_t)w_hi | (uintptr_t)w_lo | (uintptr_t)res_hi | (uintptr_t)res_lo) & 15) return LVQ_EUNSUPPORTED;
    ConvArgs a;
    a.in_hi = in_hi; a.in_lo = in_lo; a.w_hi = w_hi; a.w_lo = w_lo; a.scale = scale; a.shift = shift;
    a.out_hi = out_hi; a.out_lo = out_lo; a.out_f32 = out_f32;
    a.h = h; a.w = w; a.cp = pad32(c_in);
    a.oh = lvq_conv2d_out_size(h, kernel, stride); a.ow = lvq_conv2d_out_size(w, kernel, stride);
    if (a.oh <= 0 || a.ow <= 0) return LVQ_EINVAL;                      // kernel = stride larger than the canvas: no output pixel
    a.n_total = c_out * ups * ups; a.c_out = c_out; a.ups = ups;
    a.c_total = out_c_total; a.c_off = out_c_off; a.relu = relu;
    a.tiles_x = (int)lvq_cdiv(a.ow, TW);
    const int64_t tiles = (int64_t)a.tiles_x * lvq_cdiv(a.oh, TH);
    if (tiles >= (1ll << 31)) return LVQ_EUNSUPPORTED;
    const dim3 grid((unsigned)tiles, (unsigned)(a.n_total / BN), (unsigned)batch);
    hipStream_t st = lvq_s(stream);
    const bool split = w_lo != nullptr, wide = a.cp % 64 == 0;
    if (kernel == 3 && stride == 1) { if (wide) launch_split<3, 1, 64>(split, grid, st, a, res_hi, res_lo); else launch_split<3, 1, 32>(split, grid, st, a, res_hi, res_lo); }
    else if (kernel == 3) launch_split<3, 2, 32>(split, grid, st, a, res_hi, res_lo);
    else if (kernel == 1) { if (wide) launch_split<1, 1, 64>(split, grid, st, a, res_hi, res_lo); else launch_split<1, 1, 32>(split, grid, st, a, res_hi, res_lo); }
    else if (kernel == 2) { if (wide) launch_split<2, 2, 64>(split, grid, st, a, res_hi, res_lo); else launch_split<2, 2, 32>(split, grid, st, a, res_hi, res_lo); }
    else { if (wide) launch_split<4, 4, 64>(split, grid, st, a, res_hi, res_lo); else launch_split<4, 4, 32>(split, grid, st, a, res_hi, res_lo); }
    return lvq_launch_status();
}

}  // namespace

extern "C" int lvq_conv2d_out_size(int in, int kernel, int stride) {
    if (in <= 0 || kernel <= 0 || stride <= 0) return LVQ_EINVAL;
    if (!geom_ok(kernel, stride)) return LVQ_EUNSUPPORTED;
    return kernel == 3 ? (in - 1) / stride + 1 : in / stride;
}

extern "C" size_t lvq_conv2d_plane_elems(int batch, int c, int h, int w) {
    if (batch <= 0 || h <= 0 || w <= 0 || !cin_ok(c)) return 0;
    return (size_t)batch * h * w * pad32(c);
}

extern "C" int lvq_conv2d_to_planes(const float *x, int batch, int c, int h, int w, lvq_bf16 *hi, lvq_bf16 *lo, lvq_stream_t stream) {
    if (!x || !hi || batch <= 0 || c <= 0 || h <= 0 || w <= 0) return LVQ_EINVAL;
    if (!cin_ok(c) || batch > 65535) return LVQ_EUNSUPPORTED;
    if (((uintptr_t)hi | (uintptr_t)lo) & 15) return LVQ_EUNSUPPORTED;
    const int64_t hw = (int64_t)h * w;
    if (lvq_cdiv(hw, 64) >= (1ll << 31)) return LVQ_EUNSUPPORTED;
    const int cp = pad32(c);
    hipLaunchKernelGGL(k_to_planes, dim3((unsigned)lvq_cdiv(hw, 64), (unsigned)(cp / 32), (unsigned)batch), dim3(256), 0, lvq_s(stream), x, c, hw, cp, hi,
                       lo);
    return lvq_launch_status();
}

extern "C" size_t lvq_conv2d_packed_elems(int c_out, int c_in, int kernel, int transposed) {
    if (!cin_ok(c_in) || !cout_ok(c_out)) return 0;
    if (transposed ? !(kernel == 1 || kernel == 2 || kernel == 4) : !(kernel >= 1 && kernel <= 4)) return 0;
    return (size_t)pad32(c_in) * kernel * kernel * c_out;
}

extern "C" int lvq_conv2d_pack_weights(const float *weight, int c_out, int c_in, int kernel, int transposed, lvq_bf16 *w_hi, lvq_bf16 *w_lo,
                                       lvq_stream_t stream) {
    if (!weight || !w_hi || c_out <= 0 || c_in <= 0 || kernel <= 0) return LVQ_EINVAL;
    const int64_t n = (int64_t)lvq_conv2d_packed_elems(c_out, c_in, kernel, transposed);
    if (n == 0) return LVQ_EUNSUPPORTED;
    hipLaunchKernelGGL(k_pack_w2d, dim3((unsigned)lvq_cdiv(n, 256)), dim3(256), 0, lvq_s(stream), weight, c_out, c_in, kernel, transposed ? 1 : 0, n, w_hi,
                       w_lo);
    return lvq_launch_status();
}

extern "C" int lvq_conv2d(const lvq_bf16 *in_hi, const lvq_bf16 *in_lo, int batch, int h, int w, int c_in, const lvq_bf16 *w_hi, const lvq_bf16 *w_lo,
                          int c_out, int kernel, int stride, const float *scale, const float *shift, int relu, lvq_bf16 *out_hi, lvq_bf16 *out_lo,
                          float *out_f32, int out_c_total, int out_c_off, lvq_stream_t stream) {
    return run_conv(in_hi, in_lo, batch, h, w, c_in, w_hi, w_lo, c_out, kernel, stride, 1, scale, shift, relu, out_hi, out_lo, out_f32, out_c_total,
                    out_c_off, stream);
}

extern "C" int lvq_conv2d_res(const lvq_bf16 *in_hi, const lvq_bf16 *in_lo, int batch, int h, int w, int c_in, const lvq_bf16 *w_hi, const lvq_bf16 *w_lo,
                              int c_out, int kernel, int stride, const float *scale, const float *shift, const lvq_bf16 *res_hi, const lvq_bf16 *res_lo,
                              int relu, lvq_bf16 *out_hi, lvq_bf16 *out_lo, float *out_f32, int out_c_total, int out_c_off, lvq_stream_t stream) {
    if (!res_hi || (res_lo && !w_lo)) return LVQ_EINVAL;                // no residual at all, or a lo plane in the plain form
    return run_conv(in_hi, in_lo, batch, h, w, c_in, w_hi, w_lo, c_out, kernel, stride, 1, scale, shift, relu, out_hi, out_lo, out_f32, out_c_total,
                    out_c_off, stream, res_hi, res_lo);
}

extern "C" int lvq_deconv2d(const lvq_bf16 *in_hi, const lvq_bf16 *in_lo, int batch, int h, int w, int c_in, const lvq_bf16 *w_hi, const lvq_bf16 *w_lo,
                            int c_out, int stride, const float *scale, const float *shift, int relu, lvq_bf16 *out_hi, lvq_bf16 *out_lo, float *out_f32,
                            int out_c_total, int out_c_off, lvq_stream_t stream) {
    if (stride <= 0) return LVQ_EINVAL;
    if (!(stride == 1 || stride == 2 || stride == 4)) return LVQ_EUNSUPPORTED;
    return run_conv(in_hi, in_lo, batch, h, w, c_in, w_hi, w_lo, c_out, 1, 1, stride, scale, shift, relu, out_hi, out_lo, out_f32, out_c_total,
                    out_c_off, stream);
}
