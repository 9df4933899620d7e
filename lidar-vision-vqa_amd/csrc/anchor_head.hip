// csrc/anchor_head.hip -- the box generation and post-processing of AnchorHeadSingle (pcdet/models/dense_heads/anchor_head_template.py:225-272,
// models/model_utils/model_nms_utils.py:6-25, detectors/detector3d_template.py:178-283) for gfx950, wave64:
//
//   k_anchor_decode    generate_predicted_boxes for EVERY anchor: ResidualCoder.decode_torch, the direction classifier's bin, max_k sigmoid
//                      and its argmax.  A workgroup of 256 threads takes up to 64 consecutive pixels of the flattened map and all their
//                      anchors.  A lane reads one (pixel, anchor): neighbouring lanes read neighbouring pixels of one channel plane, so
//                      every global load is coalesced.  The tile's anchors are first copied into LDS (a contiguous run of the anchor
//                      tensor); the decoded boxes replace them there, the logits, scores and labels go next to them, and each of the four
//                      outputs -- a contiguous run per tile, since the flat anchor order is (y, x, a) -- leaves as 16-byte vectors.  The
//                      optional candidate set is appended per workgroup: ds atomics for the slot inside the tile, one global atomic add
//                      per tile that has candidates.
//   k_anchor_select    class_agnostic_nms up to the NMS call.  One workgroup of 1024 threads per scene: count, radix select, bitonic
//                      sort of up to 4096 (key << 32 | ~anchor) words in 32 KB of LDS (select_sort_unordered of head_common.h), gather.
//                      With a candidate list it reads the list, else it scans all anchors; both routes run the same selection, whose
//                      result does not depend on the order of its input, so they return the same bits.
//   lvq_nms_bev_wide   head_common.h's k_nms_mask and k_nms_walk<64>: up to 64 x 64 tiles per group and a [64][64] word tile in LDS.
//
// Every store below is an ordinary vector store from C++; LDS and global counters use integer atomics.
#include "head_common.h"

#include <cmath>

namespace {

constexpr int ADEC_THREADS = 256;
constexpr int ADEC_PIXELS = 64;                   // pixels per workgroup; halved while the tile does not fit ADEC_LDS
constexpr int ADEC_LDS = 48 * 1024;
constexpr int ASEL_THREADS = 1024;
constexpr int ASEL_MAX_K = 4096;                  // NMS_PRE_MAXSIZE of every AnchorHeadSingle configuration; the walk's 64 mask words
constexpr int WIDE_WORDS = ASEL_MAX_K / 64;
constexpr int MAX_CLASSES = 64;

struct AnchorArgs {
    int c_total, A, n_cls, n_bins, cls_off, box_off, dir_off;
    int64_t hw;
    float dir_offset, dir_limit_offset, period, thresh;
};

size_t adec_lds_bytes(int px, int A, int n_cls) { return (size_t)px * A * (7 + n_cls + 3) * 4 + 16; }

// count words src[0 .. count) of LDS -> dst, a contiguous run: scalars up to the first 16-byte boundary of dst, float4 behind it
__device__ void store_run(float *__restrict__ dst, const float *src, int count) {
    const int tid = threadIdx.x;
    const int head = min(count, (int)((4u - (unsigned)(((uintptr_t)dst >> 2) & 3u)) & 3u));
    if (tid < head) dst[tid] = src[tid];
    const int body = (count - head) >> 2;
    float4 *d4 = reinterpret_cast<float4 *>(dst + head);
    for (int i = tid; i < body; i += ADEC_THREADS) {
        const float *s = src + head + 4 * i;
        d4[i] = make_float4(s[0], s[1], s[2], s[3]);
    }
    const int done = head + 4 * body;
    if (tid < count - done) dst[done + tid] = src[done + tid];
}

__global__ __launch_bounds__(ADEC_THREADS) void k_anchor_decode(const float *__restrict__ maps, const float *__restrict__ anchors, AnchorArgs a,
                                                                 int px, float *__restrict__ cls_preds, float *__restrict__ box_preds,
                                                                 float *__restrict__ scores, int32_t *__restrict__ labels,
                                                                 int32_t *__restrict__ cand, int32_t *__restrict__ cand_count) {
    extern __shared__ __align__(16) float lds[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int A = a.A, n_cls = a.n_cls;
    const int64_t hw = a.hw, p0 = (int64_t)blockIdx.x * px, N = hw * A, n0 = p0 * A;
    const int np = (int)min((int64_t)px, hw - p0), items = np * A;
    float *box_l = lds, *cls_l = box_l + (size_t)px * A * 7, *sc_l = cls_l + (size_t)px * A * n_cls;
    int32_t *lb_l = reinterpret_cast<int32_t *>(sc_l + (size_t)px * A), *cand_l = lb_l + (size_t)px * A;
    uint32_t *ctr = reinterpret_cast<uint32_t *>(cand_l + (size_t)px * A);
    for (int e = tid; e < items * 7; e += ADEC_THREADS) box_l[e] = anchors[n0 * 7 + e];
    if (tid == 0) ctr[0] = 0;
    __syncthreads();
    const float *scene = maps + (int64_t)b * a.c_total * hw + p0;
    for (int it = tid; it < items; it += ADEC_THREADS) {
        const int an = it / np, pixel = it - an * np, o = pixel * A + an;
        const float *at = scene + pixel;
        // ---- max_k sigmoid and its lowest argmax; a NaN wins and stays, as torch.max has it
        float best = 0.f;
        int lab = 0;
        for (int k = 0; k < n_cls; ++k) {
            const float v = at[(int64_t)(a.cls_off + an * n_cls + k) * hw];
            cls_l[o * n_cls + k] = v;
            const float sg = 1.0f / (1.0f + expf(-v));
            if (k == 0) best = sg;
            else if (best == best && (sg > best || sg != sg)) { best = sg; lab = k; }
        }
        // ---- ResidualCoder.decode_torch (box_coder_utils.py:45-80), each step rounded to fp32
        float t[7], an7[7];
        for (int d = 0; d < 7; ++d) { t[d] = at[(int64_t)(a.box_off + an * 7 + d) * hw]; an7[d] = box_l[o * 7 + d]; }
        const float diag = sqrtf(an7[3] * an7[3] + an7[4] * an7[4]);
        float bx[7];
        bx[0] = t[0] * diag + an7[0];
        bx[1] = t[1] * diag + an7[1];
        bx[2] = t[2] * an7[5] + an7[2];
        for (int d = 3; d < 6; ++d) bx[d] = expf(t[d]) * an7[d];
        float r = t[6] + an7[6];
        if (a.dir_off >= 0) {                                    // anchor_head_template.py:254-265
            int bin = 0;
            float top = at[(int64_t)(a.dir_off + an * a.n_bins) * hw];
            for (int j = 1; j < a.n_bins; ++j) {
                const float v = at[(int64_t)(a.dir_off + an * a.n_bins + j) * hw];
                if (top == top && (v > top || v != v)) { top = v; bin = j; }
            }
            const float v = r - a.dir_offset;
            const float rot = v - floorf(v / a.period + a.dir_limit_offset) * a.period;
            r = rot + a.dir_offset + a.period * (float)bin;
        }
        bx[6] = r;
        for (int d = 0; d < 7; ++d) box_l[o * 7 + d] = bx[d];
        sc_l[o] = best;
        lb_l[o] = lab;
        if (cand && best >= a.thresh) cand_l[atomicAdd(&ctr[0], 1u)] = (int32_t)(n0 + o);        // a NaN fails the comparison
    }
    __syncthreads();
    const int64_t row0 = (int64_t)b * N + n0;
    store_run(box_preds + row0 * 7, box_l, items * 7);
    store_run(cls_preds + row0 * n_cls, cls_l, items * n_cls);
    store_run(scores + row0, sc_l, items);
    store_run(reinterpret_cast<float *>(labels + row0), reinterpret_cast<const float *>(lb_l), items);
    if (cand) {                                                  // (workgroup-uniform)
        const uint32_t mine = ctr[0];
        if (tid == 0 && mine) ctr[1] = (uint32_t)atomicAdd(&cand_count[b], (int32_t)mine);
        __syncthreads();
        if (mine) {
            const int64_t base = (int64_t)b * N + ctr[1];
            for (uint32_t i = tid; i < mine; i += ADEC_THREADS) cand[base + i] = cand_l[i];
        }
    }
}

__global__ __launch_bounds__(ASEL_THREADS) void k_anchor_select(const float *__restrict__ scores, const int32_t *__restrict__ labels,
                                                                 const float *__restrict__ boxes, int N, int has_thresh, float thresh,
                                                                 int pre_max, const int32_t *__restrict__ cand,
                                                                 const int32_t *__restrict__ cand_count, float *__restrict__ sel_boxes,
                                                                 float *__restrict__ sel_scores, int32_t *__restrict__ sel_labels,
                                                                 int32_t *__restrict__ sel_index, int32_t *__restrict__ sel_count,
                                                                 uint32_t *__restrict__ keys_ws, int64_t keys_pitch) {
    __shared__ SelectLds<ASEL_THREADS, ASEL_MAX_K> s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *sc = scores + (int64_t)b * N;
    const int32_t *list = cand ? cand + (int64_t)b * N : nullptr;
    const int n = list ? max(0, min(cand_count[b], N)) : N;
    auto index_at = [=](int i) { return list ? list[i] : i; };
    // the key of position i, 0 when it is no candidate: an index outside the scene, a score below the threshold, a NaN under a threshold
    auto key_at = [=](int i) {
        const int idx = list ? list[i] : i;
        if ((unsigned)idx >= (unsigned)N) return 0u;
        const float v = sc[idx];
        return (!has_thresh || v >= thresh) ? key_of(v) : 0u;
    };
    if (tid == 0) s.ncand = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (int i = tid; i < n; i += ASEL_THREADS) mine += key_at(i) != 0u;
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d);
    if ((tid & 63) == 0 && mine) atomicAdd(&s.ncand, mine);
    __syncthreads();
    const int K = (int)min((uint32_t)pre_max, s.ncand);
    __syncthreads();
    if (K > 0)                                                   // (workgroup-uniform)
        select_sort_unordered<ASEL_THREADS, ASEL_MAX_K, true>(s, key_at, index_at, keys_ws + (int64_t)b * keys_pitch, n, K);
    const int64_t row0 = (int64_t)b * pre_max;
    for (int r = tid; r < pre_max; r += ASEL_THREADS) {
        float bx[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, v = 0.f;
        int32_t lab = 0, idx = -1;
        if (r < K) {
            idx = (int32_t)(0xffffffffu - (uint32_t)(s.buf[r] & 0xffffffffu));
            const int64_t from = (int64_t)b * N + idx;
            for (int d = 0; d < 7; ++d) bx[d] = boxes[from * 7 + d];
            v = scores[from];
            lab = labels[from];
        }
        for (int d = 0; d < 7; ++d) sel_boxes[(row0 + r) * 7 + d] = bx[d];
        sel_scores[row0 + r] = v;
        sel_labels[row0 + r] = lab;
        sel_index[row0 + r] = idx;
    }
    if (tid == 0) sel_count[b] = K;
}

}  // namespace

extern "C" int lvq_anchor_decode(const float *maps, int batch, int c_total, int h, int w, int cls_channel, int box_channel, int dir_channel,
                                 int n_anchors, int n_cls, int n_dir_bins, float dir_offset, float dir_limit_offset, const float *anchors,
                                 float score_thresh, float *cls_preds, float *box_preds, float *scores, int32_t *labels, int32_t *cand,
                                 int32_t *cand_count, lvq_stream_t stream) {
    if (!maps || !anchors || !cls_preds || !box_preds || !scores || !labels || batch <= 0 || c_total <= 0 || h <= 0 || w <= 0 || n_anchors <= 0 ||
        n_cls <= 0 || (cand == nullptr) != (cand_count == nullptr))
        return LVQ_EINVAL;
    if (n_cls > MAX_CLASSES) return LVQ_EUNSUPPORTED;
    const int64_t hw = (int64_t)h * w;
    if (hw * n_anchors >= (1ll << 31) || (int64_t)n_anchors * n_cls >= (1 << 24) || batch > 65535) return LVQ_EUNSUPPORTED;
    if (cls_channel < 0 || box_channel < 0 || dir_channel < -1 || (int64_t)cls_channel + (int64_t)n_anchors * n_cls > c_total ||
        (int64_t)box_channel + (int64_t)n_anchors * 7 > c_total)
        return LVQ_EINVAL;
    if (dir_channel >= 0 && (n_dir_bins <= 0 || (int64_t)dir_channel + (int64_t)n_anchors * n_dir_bins > c_total)) return LVQ_EINVAL;
    int px = ADEC_PIXELS;
    while (px > 1 && adec_lds_bytes(px, n_anchors, n_cls) > (size_t)ADEC_LDS) px >>= 1;
    if (adec_lds_bytes(px, n_anchors, n_cls) > (size_t)ADEC_LDS) return LVQ_EUNSUPPORTED;
    AnchorArgs a;
    a.c_total = c_total; a.A = n_anchors; a.n_cls = n_cls; a.n_bins = n_dir_bins; a.cls_off = cls_channel; a.box_off = box_channel;
    a.dir_off = dir_channel; a.hw = hw; a.dir_offset = dir_offset; a.dir_limit_offset = dir_limit_offset;
    a.period = dir_channel >= 0 ? (float)(2.0 * M_PI / (double)n_dir_bins) : 0.f;
    a.thresh = score_thresh;
    hipStream_t st = lvq_s(stream);
    if (cand_count) hipMemsetAsync(cand_count, 0, (size_t)batch * sizeof(int32_t), st);
    hipLaunchKernelGGL(k_anchor_decode, dim3((unsigned)lvq_cdiv(hw, px), (unsigned)batch), dim3(ADEC_THREADS),
                       adec_lds_bytes(px, n_anchors, n_cls), st, maps, anchors, a, px, cls_preds, box_preds, scores, labels, cand, cand_count);
    return lvq_launch_status();
}

extern "C" int lvq_anchor_select_workspace_bytes(int batch, int64_t n, size_t *bytes) {
    if (!bytes || batch <= 0 || n <= 0) return LVQ_EINVAL;
    if (n >= (1ll << 31) || batch > 65535) return LVQ_EUNSUPPORTED;
    LvqSizer s;
    s.take<uint32_t>((size_t)batch * (size_t)lvq_align((size_t)n * 4, 256) / 4);
    *bytes = s.total();
    return LVQ_OK;
}

extern "C" int lvq_anchor_select(const float *scores, const int32_t *labels, const float *box_preds, int batch, int64_t n, int has_thresh,
                                 float score_thresh, int pre_max, const int32_t *cand, const int32_t *cand_count, float *sel_boxes,
                                 float *sel_scores, int32_t *sel_labels, int32_t *sel_index, int32_t *sel_count, void *ws, size_t ws_bytes,
                                 lvq_stream_t stream) {
    if (!scores || !labels || !box_preds || !sel_boxes || !sel_scores || !sel_labels || !sel_index || !sel_count || batch <= 0 || n <= 0 ||
        pre_max <= 0 || (cand == nullptr) != (cand_count == nullptr) || (cand && !has_thresh))
        return LVQ_EINVAL;
    if (pre_max > ASEL_MAX_K) return LVQ_EUNSUPPORTED;
    size_t need = 0;
    const int rc = lvq_anchor_select_workspace_bytes(batch, n, &need);
    if (rc != LVQ_OK) return rc;
    if (!ws || ws_bytes < need) return LVQ_EWORKSPACE;
    const int64_t pitch = (int64_t)(lvq_align((size_t)n * 4, 256) / 4);
    LvqArena arena(ws, ws_bytes);
    uint32_t *keys = arena.take<uint32_t>((size_t)batch * pitch);
    if (!arena.ok) return LVQ_EWORKSPACE;
    hipLaunchKernelGGL(k_anchor_select, dim3((unsigned)batch), dim3(ASEL_THREADS), 0, lvq_s(stream), scores, labels, box_preds, (int)n,
                       has_thresh ? 1 : 0, score_thresh, pre_max, cand, cand_count, sel_boxes, sel_scores, sel_labels, sel_index, sel_count, keys,
                       pitch);
    return lvq_launch_status();
}

extern "C" int lvq_nms_bev_wide_workspace_bytes(int groups, int n_max, size_t *bytes) {
    if (!bytes || groups <= 0 || n_max <= 0) return LVQ_EINVAL;
    if (n_max > ASEL_MAX_K || groups > 65535) return LVQ_EUNSUPPORTED;
    LvqSizer s;
    s.take<uint64_t>((size_t)groups * n_max * nms_words(n_max));
    *bytes = s.total();
    return LVQ_OK;
}

extern "C" int lvq_nms_bev_wide(const float *boxes, int box_stride, const int32_t *counts, int groups, int n_max, int pre_max, int post_max,
                                float thresh, int32_t *keep, int32_t *keep_count, void *ws, size_t ws_bytes, lvq_stream_t stream) {
    if (!boxes || !counts || !keep || !keep_count || groups <= 0 || n_max <= 0 || pre_max <= 0 || post_max <= 0 || box_stride < 7)
        return LVQ_EINVAL;
    size_t need = 0;
    const int rc = lvq_nms_bev_wide_workspace_bytes(groups, n_max, &need);
    if (rc != LVQ_OK) return rc;
    if (!ws || ws_bytes < need) return LVQ_EWORKSPACE;
    return nms_launch<WIDE_WORDS>(boxes, box_stride, counts, groups, n_max, pre_max, post_max, thresh, keep, keep_count, ws, ws_bytes, stream);
}
