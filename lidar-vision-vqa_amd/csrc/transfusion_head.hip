// csrc/transfusion_head.hip -- the query side of TransFusionHead (pcdet/models/dense_heads/transfusion_head.py:151-218, 397-479 with
// model_utils/transfusion_utils.py:10-101) for gfx950, wave64.  The dense side (shared_conv, heatmap_head, the K | V projection of the BEV
// key stream, the two attentions, the projections and the first two norms) runs on lvq_conv2d, lvq_gemm_bf16, lvq_attention_bf16 and
// lvq_layernorm; what has no entry point there is here:
//
//   k_tf_proposals     transfusion_head.py:161-185.  One workgroup of 1024 threads per scene: heat = sigmoid(logit), the 3 x 3 local-maximum
//                      test in the sigmoid domain (a plateau keeps all its equal cells; the border of a 3 x 3 class never survives, a
//                      "point" class keeps every cell), the radix select + bitonic sort of head_common.h over n_cls * H * W, and the
//                      post-suppression heat of every class at the chosen cells (query_heatmap_score).
//   k_tf_pos_embed     transfusion_utils.py:10-26, PositionEmbeddingLearned: Conv1d(2 -> d), folded BatchNorm1d, ReLU, Conv1d(d -> d_out)
//                      (d_out = d for the module itself; the key table folded through the K | V projection has d_out = 2 d).
//   k_tf_gather        transfusion_head.py:186-204: the P feature rows out of the conv planes, the class column of class_encoding, the
//                      positions, the labels.
//   k_tf_add_cast      x + pe as a GEMM operand (bf16 hi, optional lo): with_pos_embed of transfusion_utils.py:64-65.
//   k_tf_tail          transfusion_utils.py:95-97 (linear1, ReLU, linear2, residual, norm3), SeparateHead_Transfusion
//                      (transfusion_head.py:15-49) and the arithmetic of get_bboxes / decode_bbox (455-479, 397-416) for 8 query rows per
//                      workgroup, fp32 FMA chains in ascending k.
//   k_tf_compact       decode_bbox's masks (433-451): the kept rows of a scene in proposal order.  A launch of its own because the
//                      rank of a row is a prefix over the scene's P rows, which k_tf_tail spreads over P / 8 workgroups.
//
// The grid's geometry (CenterGeom), the range-and-threshold mask (box_stays, with the threshold always applied) and the compaction
// (compact_store) are head_common.h's, shared with center_head.hip; the box arithmetic is this head's own (the sine comes first in rot).
//
// Order of the proposals: the fp32 heat, descending, equal values towards the LOWER flat index class * H * W + cell (the reference's
// argsort leaves ties open); NaN first (head_common.h: key_of).  A NaN heat stays NaN whatever its neighbours (NaN * 0 in the reference),
// and a cell with a NaN neighbour is suppressed (max_pool2d hands the NaN on, and nothing equals it).
//
// Every store below is an ordinary vector store from C++; LDS counters use ds atomics.
#include "head_common.h"

namespace {

constexpr int PROP_THREADS = 1024;
constexpr int MAX_P = 1024;            // the sort buffer; also k_tf_compact's one row per thread
constexpr int MAX_CLS = 64;            // bits of the point-class mask
constexpr int TF_D = 128;              // HIDDEN_CHANNEL of the tail
constexpr int TF_HC = 64;              // head_channels of SeparateHead_Transfusion
constexpr int MAX_FFN = 512;
constexpr int MAX_BRANCH = 6;
constexpr int TAIL_ROWS = 8;
constexpr int TAIL_THREADS = 256;
constexpr int MAX_CT = 10 + MAX_CLS;   // output channels of the six branches
constexpr int PE_ROWS = 8;
constexpr int PE_THREADS = 128;
constexpr int PE_MAX_D = 512;

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// heatmap * (heatmap == local_max) of transfusion_head.py:162-177 at one cell of one class plane
__device__ __forceinline__ float heat_at(const float *__restrict__ plane, int y, int x, int h, int w, bool point) {
    const float v = sigm(plane[y * w + x]);
    if (v != v || point) return v;
    if (y == 0 || x == 0 || y == h - 1 || x == w - 1) return 0.f;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const float o = sigm(plane[(y + dy) * w + (x + dx)]);
            if (!(o <= v)) return 0.f;
        }
    return v;
}

__global__ __launch_bounds__(PROP_THREADS) void k_tf_proposals(const float *__restrict__ maps, int c_total, int first, int n_cls, int h, int w,
                                                                uint64_t point_mask, int P, int32_t *__restrict__ prop_flat,
                                                                float *__restrict__ prop_score, float *__restrict__ qhs,
                                                                uint32_t *__restrict__ keys_ws, int64_t keys_pitch) {
    __shared__ SelectLds<PROP_THREADS, MAX_P> s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int hw = h * w, n = n_cls * hw;
    const float *hm = maps + ((int64_t)b * c_total + first) * hw;
    select_sort<PROP_THREADS, MAX_P, false>(s, [=](int i) {
        const int cls = i / hw, pix = i - cls * hw, y = pix / w, x = pix - y * w;
        return key_of(heat_at(hm + (int64_t)cls * hw, y, x, h, w, (point_mask >> cls) & 1ull));
    }, keys_ws + (int64_t)b * keys_pitch, n, P);
    if (tid < P) {
        const uint64_t e = s.buf[tid];
        prop_flat[(int64_t)b * P + tid] = (int32_t)(0xffffffffu - (uint32_t)(e & 0xffffffffu));
        prop_score[(int64_t)b * P + tid] = score_of((uint32_t)(e >> 32));
    }
    for (int e = tid; e < n_cls * P; e += PROP_THREADS) {
        const int cls = e / P, p = e - cls * P;
        const uint32_t idx = 0xffffffffu - (uint32_t)(s.buf[p] & 0xffffffffu);
        const int pix = (int)(idx % (uint32_t)hw), y = pix / w, x = pix - y * w;
        qhs[((int64_t)b * n_cls + cls) * P + p] = heat_at(hm + (int64_t)cls * hw, y, x, h, w, (point_mask >> cls) & 1ull);
    }
}

// rows [row0, row0 + PE_ROWS) of pos [n, 2] -> out [n, d_out]
__global__ __launch_bounds__(PE_THREADS) void k_tf_pos_embed(const float *__restrict__ pos, int64_t n, int d, int d_out, const float *__restrict__ w1,
                                                              const float *__restrict__ scale, const float *__restrict__ shift,
                                                              const float *__restrict__ w2, const float *__restrict__ b2,
                                                              float *__restrict__ out) {
    __shared__ float ps[PE_ROWS][2];
    __shared__ float hs[PE_ROWS][PE_MAX_D];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * PE_ROWS;
    const int rows = (int)min((int64_t)PE_ROWS, n - row0);
    if (tid < PE_ROWS * 2) ps[tid >> 1][tid & 1] = (tid >> 1) < rows ? pos[(row0 + (tid >> 1)) * 2 + (tid & 1)] : 0.f;
    __syncthreads();
    for (int j = tid; j < d; j += PE_THREADS) {
        const float wx = w1[2 * j], wy = w1[2 * j + 1], sc = scale[j], sh = shift[j];
        for (int r = 0; r < PE_ROWS; ++r) hs[r][j] = fmaxf(fmaf(fmaf(wy, ps[r][1], wx * ps[r][0]), sc, sh), 0.f);
    }
    __syncthreads();
    for (int j = tid; j < d_out; j += PE_THREADS) {
        float acc[PE_ROWS];
        for (int r = 0; r < PE_ROWS; ++r) acc[r] = 0.f;
        const float4 *wr = (const float4 *)(w2 + (int64_t)j * d);
        for (int k = 0; k < d; k += 4) {
            const float4 wv = wr[k >> 2];
            for (int r = 0; r < PE_ROWS; ++r) {
                acc[r] = fmaf(wv.x, hs[r][k], acc[r]);
                acc[r] = fmaf(wv.y, hs[r][k + 1], acc[r]);
                acc[r] = fmaf(wv.z, hs[r][k + 2], acc[r]);
                acc[r] = fmaf(wv.w, hs[r][k + 3], acc[r]);
            }
        }
        const float bj = b2[j];
        for (int r = 0; r < rows; ++r) out[(row0 + r) * d_out + j] = acc[r] + bj;
    }
}

// one query row per workgroup
__global__ __launch_bounds__(128) void k_tf_gather(const uint16_t *__restrict__ hi, const uint16_t *__restrict__ lo, int hw, int d, int n_cls,
                                                    int y_size, int P, const int32_t *__restrict__ prop_flat, const float *__restrict__ class_w,
                                                    const float *__restrict__ class_b, float *__restrict__ query_feat,
                                                    float *__restrict__ query_pos, int32_t *__restrict__ query_labels) {
    const int64_t row = blockIdx.x;
    const int b = (int)(row / P), tid = threadIdx.x;
    const int flat = max(0, min(prop_flat[row], n_cls * hw - 1));            // never index with a stray entry
    const int cls = flat / hw, pix = flat - cls * hw;
    const int64_t src = ((int64_t)b * hw + pix) * d;
    for (int j = tid; j < d; j += 128) {
        float v = bf16_to_f32(hi[src + j]);
        if (lo) v += bf16_to_f32(lo[src + j]);
        query_feat[row * d + j] = v + (class_w[(int64_t)j * n_cls + cls] + class_b[j]);
    }
    if (tid == 0) {
        // the reference's own formula (create_2D_grid is an `ij` meshgrid over (x_size, y_size), indexed with the row-major cell)
        query_pos[row * 2] = (float)(pix % y_size) + 0.5f;
        query_pos[row * 2 + 1] = (float)(pix / y_size) + 0.5f;
        query_labels[row] = cls;
    }
}

__global__ __launch_bounds__(256) void k_tf_add_cast(const float *__restrict__ x, const float *__restrict__ pe, int64_t n,
                                                      uint16_t *__restrict__ hi, uint16_t *__restrict__ lo) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = x[i] + pe[i];
    const uint16_t h = f32_to_bf16(v);
    hi[i] = h;
    if (lo) lo[i] = f32_to_bf16(v - bf16_to_f32(h));
}

struct TailW {
    const float *w1, *b1, *w2, *b2, *gamma, *beta;      // linear1 [F, 128], linear2 [128, F], norm3
    const float *hw1, *hscale, *hshift;                 // first convs [nb * 64, 128], folded norm [nb * 64]
    const float *hw2, *hb2;                             // last convs [c_total, 64], bias [c_total]
    int ffn, nb, n_cls, c_total, c_box;
    float eps;
};
__device__ __forceinline__ int branch_of(int o, int c_box, int nb) {
    if (o >= c_box) return nb - 1;
    return o < 2 ? 0 : o < 3 ? 1 : o < 6 ? 2 : o < 8 ? 3 : 4;
}

// acc[r] += sum_k w[k] * xs[r][k], k ascending, for ROWS rows of an LDS tile with row pitch `pitch`
template <int ROWS>
__device__ __forceinline__ void dot_rows(const float *__restrict__ wrow, const float *xs, int pitch, int K, float *acc) {
    const float4 *wr = (const float4 *)wrow;
    for (int k = 0; k < K; k += 4) {
        const float4 wv = wr[k >> 2];
        for (int r = 0; r < ROWS; ++r) {
            const float *xr = xs + r * pitch + k;
            acc[r] = fmaf(wv.x, xr[0], acc[r]);
            acc[r] = fmaf(wv.y, xr[1], acc[r]);
            acc[r] = fmaf(wv.z, xr[2], acc[r]);
            acc[r] = fmaf(wv.w, xr[3], acc[r]);
        }
    }
}

__global__ __launch_bounds__(TAIL_THREADS) void k_tf_tail(const float *__restrict__ x, const float *__restrict__ qpos,
                                                           const int32_t *__restrict__ qlabels, const float *__restrict__ prop_score, int R,
                                                           int P, TailW tw, CenterGeom gm, int box_dim, float *__restrict__ raw,
                                                           float *__restrict__ tmp_boxes, float *__restrict__ tmp_scores,
                                                           int32_t *__restrict__ tmp_keep) {
    __shared__ float xs[TAIL_ROWS][TF_D];
    __shared__ float hb[TAIL_ROWS][MAX_FFN];
    __shared__ float ys[TAIL_ROWS][TF_D];
    __shared__ float ts[TAIL_ROWS][MAX_BRANCH * TF_HC];
    __shared__ float rs[TAIL_ROWS][MAX_CT];
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * TAIL_ROWS;
    const int rows = min(TAIL_ROWS, R - row0);
    for (int e = tid; e < TAIL_ROWS * TF_D; e += TAIL_THREADS) {
        const int r = e / TF_D, k = e - r * TF_D;
        xs[r][k] = r < rows ? x[(int64_t)(row0 + r) * TF_D + k] : 0.f;
    }
    __syncthreads();
    // linear1 + ReLU
    for (int j = tid; j < tw.ffn; j += TAIL_THREADS) {
        float acc[TAIL_ROWS];
        for (int r = 0; r < TAIL_ROWS; ++r) acc[r] = 0.f;
        dot_rows<TAIL_ROWS>(tw.w1 + (int64_t)j * TF_D, &xs[0][0], TF_D, TF_D, acc);
        const float bj = tw.b1[j];
        for (int r = 0; r < TAIL_ROWS; ++r) hb[r][j] = fmaxf(acc[r] + bj, 0.f);
    }
    __syncthreads();
    // linear2 + residual
    {
        const int j = tid & (TF_D - 1), half = tid >> 7;                     // 256 threads: two groups of four rows
        float acc[TAIL_ROWS / 2];
        for (int r = 0; r < TAIL_ROWS / 2; ++r) acc[r] = 0.f;
        dot_rows<TAIL_ROWS / 2>(tw.w2 + (int64_t)j * tw.ffn, &hb[half * (TAIL_ROWS / 2)][0], MAX_FFN, tw.ffn, acc);
        const float bj = tw.b2[j];
        for (int r = 0; r < TAIL_ROWS / 2; ++r) {
            const int rr = half * (TAIL_ROWS / 2) + r;
            ys[rr][j] = xs[rr][j] + (acc[r] + bj);
        }
    }
    __syncthreads();
    // norm3: centred statistics, two rows per wave
    {
        const int lane = tid & 63, wave = tid >> 6;
        for (int q = 0; q < TAIL_ROWS / 4; ++q) {
            const int r = wave * (TAIL_ROWS / 4) + q;
            const float a0 = ys[r][lane], a1 = ys[r][lane + 64];
            float sum = a0 + a1;
            for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
            const float mean = sum / (float)TF_D;
            const float d0 = a0 - mean, d1 = a1 - mean;
            float sq = d0 * d0 + d1 * d1;
            for (int d = 32; d > 0; d >>= 1) sq += __shfl_xor(sq, d);
            const float inv = 1.0f / sqrtf(sq / (float)TF_D + tw.eps);
            ys[r][lane] = d0 * inv * tw.gamma[lane] + tw.beta[lane];
            ys[r][lane + 64] = d1 * inv * tw.gamma[lane + 64] + tw.beta[lane + 64];
        }
    }
    __syncthreads();
    // first convs of the branches: folded norm + ReLU
    for (int j = tid; j < tw.nb * TF_HC; j += TAIL_THREADS) {
        float acc[TAIL_ROWS];
        for (int r = 0; r < TAIL_ROWS; ++r) acc[r] = 0.f;
        dot_rows<TAIL_ROWS>(tw.hw1 + (int64_t)j * TF_D, &ys[0][0], TF_D, TF_D, acc);
        const float sc = tw.hscale[j], sh = tw.hshift[j];
        for (int r = 0; r < TAIL_ROWS; ++r) ts[r][j] = fmaxf(fmaf(acc[r], sc, sh), 0.f);
    }
    __syncthreads();
    // last convs
    for (int e = tid; e < TAIL_ROWS * tw.c_total; e += TAIL_THREADS) {
        const int r = e / tw.c_total, o = e - r * tw.c_total;
        float acc = 0.f;
        dot_rows<1>(tw.hw2 + (int64_t)o * TF_HC, &ts[r][branch_of(o, tw.c_box, tw.nb) * TF_HC], 0, TF_HC, &acc);
        rs[r][o] = acc + tw.hb2[o];
    }
    __syncthreads();
    // res_layer: channel-major [B, c_total, P]; center carries query_pos (transfusion_head.py:210)
    for (int e = tid; e < TAIL_ROWS * tw.c_total; e += TAIL_THREADS) {
        const int o = e / TAIL_ROWS, r = e - o * TAIL_ROWS;
        if (r >= rows) continue;
        const int row = row0 + r, b = row / P, p = row - b * P;
        float v = rs[r][o];
        if (o < 2) v += qpos[(int64_t)row * 2 + o];
        raw[((int64_t)b * tw.c_total + o) * P + p] = v;
    }
    // get_bboxes + decode_bbox for one row per thread
    if (tid < rows) {
        const int row = row0 + tid;
        const float *rr = rs[tid];
        const int label = max(0, min(qlabels[row], tw.n_cls - 1));
        const float sc = sigm(rr[tw.c_box + label]) * prop_score[row];
        float bx[9];
        bx[0] = (rr[0] + qpos[(int64_t)row * 2]) * gm.stride * gm.vx + gm.rx;
        bx[1] = (rr[1] + qpos[(int64_t)row * 2 + 1]) * gm.stride * gm.vy + gm.ry;
        bx[2] = rr[2];
        for (int d = 0; d < 3; ++d) bx[3 + d] = expf(rr[3 + d]);
        bx[6] = atan2f(rr[6], rr[7]);                                          // rot[:, 0] is the SINE here (transfusion_head.py:410-411)
        bx[7] = bx[8] = 0.f;
        if (box_dim == 9) { bx[7] = rr[8]; bx[8] = rr[9]; }
        const bool keep = box_stays<false>(bx, sc, gm);                        // the threshold always counts here
        for (int d = 0; d < box_dim; ++d) tmp_boxes[(int64_t)row * box_dim + d] = bx[d];
        tmp_scores[row] = sc;
        tmp_keep[row] = keep ? 1 : 0;
    }
}

// one workgroup per scene, thread p holds proposal p
__global__ __launch_bounds__(MAX_P) void k_tf_compact(const float *__restrict__ tmp_boxes, const float *__restrict__ tmp_scores,
                                                       const int32_t *__restrict__ tmp_keep, const int32_t *__restrict__ qlabels, int P,
                                                       int box_dim, float *__restrict__ boxes, float *__restrict__ scores,
                                                       int32_t *__restrict__ labels, int32_t *__restrict__ counts) {
    __shared__ uint32_t wcnt[MAX_P / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t row = (int64_t)b * P + tid;
    const bool keep = tid < P && tmp_keep[row] != 0;
    float bx[9];
    float sc = 0.f;
    int label = 0;
    if (keep) {
        for (int d = 0; d < box_dim; ++d) bx[d] = tmp_boxes[row * box_dim + d];
        sc = tmp_scores[row];
        label = qlabels[row] + 1;                                              // get_bboxes: .int() + 1
    }
    compact_store<MAX_P>(wcnt, keep, bx, sc, label, b, P, box_dim, boxes, scores, labels, counts);
}

template <typename A>
void tail_layout(A &arena, int64_t rows, int box_dim, float *&tb, float *&tsc, int32_t *&tk) {
    tb = arena.template take<float>((size_t)rows * box_dim);
    tsc = arena.template take<float>((size_t)rows);
    tk = arena.template take<int32_t>((size_t)rows);
}

}  // namespace

extern "C" int lvq_heatmap_proposals_workspace_bytes(int batch, int n_cls, int h, int w, size_t *bytes) {
    if (!bytes || batch <= 0 || n_cls <= 0 || h <= 0 || w <= 0) return LVQ_EINVAL;
    if (n_cls > MAX_CLS) return LVQ_EINVAL;
    const int64_t n = (int64_t)n_cls * h * w;
    if (n >= (1ll << 31) || batch > 65535) return LVQ_EUNSUPPORTED;
    LvqSizer s;
    s.take<uint32_t>((size_t)batch * (size_t)lvq_align((size_t)n * 4, 256) / 4);
    *bytes = s.total();
    return LVQ_OK;
}

extern "C" int lvq_heatmap_proposals(const float *maps, int batch, int c_total, int h, int w, int first_channel, int n_cls,
                                     int64_t point_class_mask, int nms_kernel_size, int n_proposals, int32_t *prop_flat, float *prop_score,
                                     float *query_heatmap_score, void *ws, size_t ws_bytes, lvq_stream_t stream) {
    if (!maps || !prop_flat || !prop_score || !query_heatmap_score || batch <= 0 || c_total <= 0 || h <= 0 || w <= 0 || n_cls <= 0 ||
        first_channel < 0 || n_proposals <= 0 || first_channel + (int64_t)n_cls > c_total)
        return LVQ_EINVAL;
    if (n_cls > MAX_CLS || h < 3 || w < 3 || (int64_t)n_proposals > (int64_t)n_cls * h * w) return LVQ_EINVAL;
    if (n_proposals > MAX_P || nms_kernel_size != 3) return LVQ_EUNSUPPORTED;
    size_t need = 0;
    const int rc = lvq_heatmap_proposals_workspace_bytes(batch, n_cls, h, w, &need);
    if (rc != LVQ_OK) return rc;
    if (!ws || ws_bytes < need) return LVQ_EWORKSPACE;
    const int64_t pitch = (int64_t)(lvq_align((size_t)n_cls * h * w * 4, 256) / 4);
    LvqArena arena(ws, ws_bytes);
    uint32_t *keys = arena.take<uint32_t>((size_t)batch * pitch);
    if (!arena.ok) return LVQ_EWORKSPACE;
    hipLaunchKernelGGL(k_tf_proposals, dim3((unsigned)batch), dim3(PROP_THREADS), 0, lvq_s(stream), maps, c_total, first_channel, n_cls, h, w,
                       (uint64_t)point_class_mask, n_proposals, prop_flat, prop_score, query_heatmap_score, keys, pitch);
    return lvq_launch_status();
}

static int pos_embed_check(int d, int d_out, const float *w1, const float *scale, const float *shift, const float *w2, const float *b2) {
    if (!w1 || !scale || !shift || !w2 || !b2 || d <= 0 || d_out <= 0) return LVQ_EINVAL;
    if ((d & 3) || d > PE_MAX_D || d_out > PE_MAX_D || ((uintptr_t)w2 & 15)) return LVQ_EUNSUPPORTED;
    return LVQ_OK;
}

extern "C" int lvq_pos_embed_learned(const float *pos, int64_t n, int d, int d_out, const float *w1, const float *scale, const float *shift,
                                     const float *w2, const float *b2, float *out, lvq_stream_t stream) {
    if (!pos || !out || n <= 0) return LVQ_EINVAL;
    const int rc = pos_embed_check(d, d_out, w1, scale, shift, w2, b2);
    if (rc != LVQ_OK) return rc;
    const int64_t blocks = lvq_cdiv(n, PE_ROWS);
    if (blocks > 0x7fffffff) return LVQ_EUNSUPPORTED;
    hipLaunchKernelGGL(k_tf_pos_embed, dim3((unsigned)blocks), dim3(PE_THREADS), 0, lvq_s(stream), pos, n, d, d_out, w1, scale, shift, w2, b2, out);
    return lvq_launch_status();
}

extern "C" int lvq_transfusion_queries(const lvq_bf16 *feat_hi, const lvq_bf16 *feat_lo, int batch, int h, int w, int d,
                                       const int32_t *prop_flat, int n_proposals, int n_cls, int y_size, const float *class_w,
                                       const float *class_b, const float *pe_w1, const float *pe_scale, const float *pe_shift,
                                       const float *pe_w2, const float *pe_b2, float *query_feat, float *query_pos, int32_t *query_labels,
                                       float *query_pe, lvq_stream_t stream) {
    if (!feat_hi || !prop_flat || !class_w || !class_b || !query_feat || !query_pos || !query_labels || !query_pe || batch <= 0 || h <= 0 ||
        w <= 0 || n_proposals <= 0 || n_cls <= 0 || y_size <= 0)
        return LVQ_EINVAL;
    const int rc = pos_embed_check(d, d, pe_w1, pe_scale, pe_shift, pe_w2, pe_b2);
    if (rc != LVQ_OK) return rc;
    if ((d & 31) || n_cls > MAX_CLS || (int64_t)n_cls * h * w >= (1ll << 31) || (int64_t)batch * n_proposals > 0x7fffffff) return LVQ_EUNSUPPORTED;
    const int64_t rows = (int64_t)batch * n_proposals;
    hipStream_t st = lvq_s(stream);
    hipLaunchKernelGGL(k_tf_gather, dim3((unsigned)rows), dim3(128), 0, st, feat_hi, feat_lo, h * w, d, n_cls, y_size, n_proposals, prop_flat,
                       class_w, class_b, query_feat, query_pos, query_labels);
    hipLaunchKernelGGL(k_tf_pos_embed, dim3((unsigned)lvq_cdiv(rows, PE_ROWS)), dim3(PE_THREADS), 0, st, (const float *)query_pos, rows, d, d,
                       pe_w1, pe_scale, pe_shift, pe_w2, pe_b2, query_pe);
    return lvq_launch_status();
}

extern "C" int lvq_transfusion_add_pe(const float *x, const float *pe, int64_t n, lvq_bf16 *hi, lvq_bf16 *lo, lvq_stream_t stream) {
    if (!x || !pe || !hi || n <= 0) return LVQ_EINVAL;
    const int64_t blocks = lvq_cdiv(n, 256);
    if (blocks > 0x7fffffff) return LVQ_EUNSUPPORTED;
    hipLaunchKernelGGL(k_tf_add_cast, dim3((unsigned)blocks), dim3(256), 0, lvq_s(stream), x, pe, n, hi, lo);
    return lvq_launch_status();
}

extern "C" int lvq_transfusion_tail_workspace_bytes(int batch, int n_proposals, int box_dim, size_t *bytes) {
    if (!bytes || batch <= 0 || n_proposals <= 0 || (box_dim != 7 && box_dim != 9)) return LVQ_EINVAL;
    if (n_proposals > MAX_P || batch > 65535) return LVQ_EUNSUPPORTED;
    SizerAdapter sz;
    float *a, *b;
    int32_t *c;
    tail_layout(sz, (int64_t)batch * n_proposals, box_dim, a, b, c);
    *bytes = sz.s.total();
    return LVQ_OK;
}

extern "C" int lvq_transfusion_tail(const float *x, const float *query_pos, const int32_t *query_labels, const float *prop_score, int batch,
                                    int n_proposals, int ffn, int n_cls, int has_vel, const float *w1, const float *b1, const float *w2,
                                    const float *b2, const float *gamma, const float *beta, float eps, const float *head_w1,
                                    const float *head_scale, const float *head_shift, const float *head_w2, const float *head_b2, int stride,
                                    const float *voxel_xy, const float *range_xy, const float *limit_range, float score_thresh, float *raw,
                                    float *boxes, float *scores, int32_t *labels, int32_t *counts, void *ws, size_t ws_bytes,
                                    lvq_stream_t stream) {
    if (!x || !query_pos || !query_labels || !prop_score || !w1 || !b1 || !w2 || !b2 || !gamma || !beta || !head_w1 || !head_scale ||
        !head_shift || !head_w2 || !head_b2 || !voxel_xy || !range_xy || !limit_range || !raw || !boxes || !scores || !labels || !counts ||
        batch <= 0 || n_proposals <= 0 || ffn <= 0 || n_cls <= 0 || stride <= 0)
        return LVQ_EINVAL;
    if (n_proposals > MAX_P || batch > 65535 || (ffn & 63) || ffn > MAX_FFN || n_cls > MAX_CLS) return LVQ_EUNSUPPORTED;
    if (((uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)head_w1 | (uintptr_t)head_w2) & 15) return LVQ_EUNSUPPORTED;
    const int box_dim = has_vel ? 9 : 7;
    size_t need = 0;
    const int rc = lvq_transfusion_tail_workspace_bytes(batch, n_proposals, box_dim, &need);
    if (rc != LVQ_OK) return rc;
    if (!ws || ws_bytes < need) return LVQ_EWORKSPACE;
    const int R = batch * n_proposals;
    LvqArena arena(ws, ws_bytes);
    float *tb, *tsc;
    int32_t *tk;
    tail_layout(arena, R, box_dim, tb, tsc, tk);
    if (!arena.ok) return LVQ_EWORKSPACE;
    TailW tw;
    tw.w1 = w1; tw.b1 = b1; tw.w2 = w2; tw.b2 = b2; tw.gamma = gamma; tw.beta = beta;
    tw.hw1 = head_w1; tw.hscale = head_scale; tw.hshift = head_shift; tw.hw2 = head_w2; tw.hb2 = head_b2;
    tw.ffn = ffn; tw.nb = has_vel ? 6 : 5; tw.n_cls = n_cls; tw.c_box = has_vel ? 10 : 8; tw.c_total = tw.c_box + n_cls; tw.eps = eps;
    const CenterGeom gm = center_geom(stride, voxel_xy, range_xy, limit_range, score_thresh);
    hipStream_t st = lvq_s(stream);
    hipLaunchKernelGGL(k_tf_tail, dim3((unsigned)lvq_cdiv(R, TAIL_ROWS)), dim3(TAIL_THREADS), 0, st, x, query_pos, query_labels, prop_score, R,
                       n_proposals, tw, gm, box_dim, raw, tb, tsc, tk);
    hipLaunchKernelGGL(k_tf_compact, dim3((unsigned)batch), dim3(MAX_P), 0, st, (const float *)tb, (const float *)tsc, (const int32_t *)tk,
                       query_labels, n_proposals, box_dim, boxes, scores, labels, counts);
    return lvq_launch_status();
}
