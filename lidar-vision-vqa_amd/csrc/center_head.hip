// csrc/center_head.hip -- the post-processing of CenterHead (pcdet/models/dense_heads/center_head.py:297-365) for gfx950, wave64:
//
//   k_center_decode    centernet_utils.py:155-241.  One workgroup of 1024 threads per (scene, task): a 4 x 8-bit radix select of the K-th
//                      largest fp32 score over n_cls * H * W, a bitonic sort of the K winners in LDS, the box arithmetic, the masks and
//                      an order-keeping compaction.  Nothing is handed between workgroups.
//   k_voxel_decode     centernet_utils.py:243-354 (VoxelNeXtHead): the same selection, sort, masks and compaction (select_sort and
//                      decode_winners are shared, not copied) over the ROWS of a sparse tensor: the candidates of a scene are the rows
//                      whose batch index is the scene's, in stored order and not necessarily contiguous; y and x come from the rows'
//                      own indices.  One deliberate difference from the reference: when a scene has fewer than K rows, _topk_1d still
//                      computes class = ind // K on an [n_cls, n_b] matrix, which gives wrong classes, and when n_cls * n_b < K its
//                      torch.stack / .view(batch, K) raise.  Here the class is the matrix row the candidate came from and the count is
//                      what there is; with n_b >= K in every scene the two agree.
//   k_boxes_iou_bev    iou3d_nms_utils.py:31-45.  One thread per (a, b) pair.
//   k_nms_mask         iou3d_nms_utils.py:120-135, first half.  One wave per 64 x 64 tile on or above the diagonal: a lane holds a
//                      column box, the rows are looped, __ballot(iou > thresh) is the row's 64-bit word.
//   k_nms_walk         second half.  One wave per group walks the rows on the device: the mask never travels to the host.
//   k_center_collect   center_head.py:352-363.  One workgroup per scene gathers the kept rows of its tasks, in head order.
//
// Order of the candidates.  The key is the fp32 score sigmoid(hm) itself, descending; a NaN of either sign sorts first, as torch.topk has
// it (all NaNs share one key, so they are ordered like any other tie; they fail `score > thresh` and are kept when there is none); equal
// scores are taken and ordered towards the LOWER flat index c * H * W + y * W + x, so the result does not depend on how threads were
// scheduled.  torch.topk leaves the order of equal scores open; the reference's two-stage top-k (per class, then over the classes'
// winners) selects the same set as this global one whenever the scores around the K-th are distinct.
//
// Rotated rectangle intersection.  Written from the geometry, not from the reference's kernel: box a's four corners are moved into box
// b's frame (the centre DIFFERENCE is rotated, so the arithmetic runs on numbers of the boxes' own size, not of the scene's), the
// quadrilateral is clipped against b's four axis-aligned half-planes (Sutherland-Hodgman; a convex polygon gains at most one vertex per
// plane, 8 in all) and the shoelace formula gives the area.  There is no corner margin: clipping is continuous in the corners, touching
// boxes give an area that rounds to zero, identical boxes the full area, and nothing has to be made robust by moving a corner.
// IoU = area / max(sa + sb - area, 1e-8), as iou3d_nms_kernel.cu:217-234 divides.
//
// The selection (key_of, select_sort), the rectangles (Rect, rect_iou), k_nms_mask / k_nms_walk, the grid's geometry (CenterGeom), the
// range-and-threshold mask (box_stays) and the compaction (compact_store) live in head_common.h, which anchor_head.hip and
// transfusion_head.hip share; this file instantiates them for 1024 threads, 1024 sort rows and 16 mask words.  What the two decode kernels
// share beyond that is here: the box arithmetic (decode_box), the tail "winner tid of the sort buffer: decode, mask, label, compact"
// (decode_winners, with the index-to-cell mapping as a callable) and, on the host, center_tables, which builds CenterTasks and CenterGeom
// from the ABI's arrays for both entry points.
//
// Every store below is an ordinary vector store from C++; LDS counters use ds atomics.
#include "head_common.h"

namespace {

constexpr int DEC_THREADS = 1024;
constexpr int MAX_K = 1024;            // the sort buffer and the walk's 16 mask words
constexpr int MAX_TASKS = 16;
constexpr int MAX_CLASSES = 64;
constexpr int NMS_WORDS = MAX_K / 64;

struct CenterTasks {                   // by value in the kernel arguments
    int off[MAX_TASKS][6];             // channel of center, center_z, dim, rot, vel (-1: none), hm
    int n_cls[MAX_TASKS];
    int map_off[MAX_TASKS];
    int cls_map[MAX_CLASSES];
};

// the box of a candidate at cell (x, y); ch(c) reads channel c at the candidate (centernet_utils.py:184-212 / 310-319)
template <class Ch>
__device__ __forceinline__ void decode_box(Ch ch, int x, int y, const int *off, const CenterGeom &gm, int box_dim, float *bx) {
    bx[0] = ((float)x + ch(off[0])) * gm.stride * gm.vx + gm.rx;
    bx[1] = ((float)y + ch(off[0] + 1)) * gm.stride * gm.vy + gm.ry;
    bx[2] = ch(off[1]);
    for (int d = 0; d < 3; ++d) bx[3 + d] = expf(ch(off[2] + d));
    bx[6] = atan2f(ch(off[3] + 1), ch(off[3]));                // rot[:, 0] is the cosine, rot[:, 1] the sine
    bx[7] = bx[8] = 0.f;
    if (box_dim == 9) { bx[7] = ch(off[4]); bx[8] = ch(off[4] + 1); }
}

// Thread tid < n_win holds winner tid of the sort buffer: its box, the masks, its label, then the compaction of the group's winners
// (centernet_utils.py:184-221 / 310-336).  locate(idx, cls, x, y) splits the flat index into the class and the cell and returns the
// reader of a channel at that candidate.  Every thread of the workgroup calls it.
template <class Locate>
__device__ __forceinline__ void decode_winners(SelectLds<DEC_THREADS, MAX_K> &s, int n_win, Locate locate, const CenterTasks &tk, int t,
                                               const CenterGeom &gm, int g, int K, int box_dim, float *__restrict__ boxes,
                                               float *__restrict__ scores, int32_t *__restrict__ labels, int32_t *__restrict__ counts) {
    bool keep = false;
    float bx[9];
    float sc = 0.f;
    int label = 0;
    if ((int)threadIdx.x < n_win) {
        const uint64_t e = s.buf[threadIdx.x];
        const uint32_t idx = 0xffffffffu - (uint32_t)(e & 0xffffffffu);
        sc = score_of((uint32_t)(e >> 32));
        int cls, x, y;
        const auto ch = locate(idx, cls, x, y);
        decode_box(ch, x, y, tk.off[t], gm, box_dim, bx);
        keep = box_stays<true>(bx, sc, gm);
        label = tk.cls_map[tk.map_off[t] + cls];
    }
    compact_store<DEC_THREADS>(s.wcnt, keep, bx, sc, label, g, K, box_dim, boxes, scores, labels, counts);
}

__global__ __launch_bounds__(DEC_THREADS) void k_center_decode(const float *__restrict__ maps, int c_total, int h, int w, int n_tasks,
                                                                CenterTasks tk, CenterGeom gm, int K, int box_dim,
                                                                float *__restrict__ boxes, float *__restrict__ scores,
                                                                int32_t *__restrict__ labels, int32_t *__restrict__ counts,
                                                                uint32_t *__restrict__ keys_ws, int64_t keys_pitch) {
    __shared__ SelectLds<DEC_THREADS, MAX_K> s;
    const int g = blockIdx.x, b = g / n_tasks, t = g - b * n_tasks;
    const int64_t hw = (int64_t)h * w;
    const int n = (int)(tk.n_cls[t] * hw);
    const float *scene = maps + (int64_t)b * c_total * hw;
    const float *hm = scene + (int64_t)tk.off[t][5] * hw;
    select_sort<DEC_THREADS, MAX_K, false>(s, [hm](int i) { return key_of(1.0f / (1.0f + expf(-hm[i]))); }, keys_ws + (int64_t)g * keys_pitch, n, K);
    decode_winners(s, K, [&](uint32_t idx, int &cls, int &x, int &y) {
        cls = (int)(idx / (uint32_t)hw);
        const int pix = (int)(idx - (uint32_t)cls * (uint32_t)hw);
        y = pix / w; x = pix - y * w;
        return [=](int c) { return scene[(int64_t)c * hw + pix]; };
    }, tk, t, gm, g, K, box_dim, boxes, scores, labels, counts);
}

// centernet_utils.py:243-354 over rows: the candidates of scene b are the rows with indices[:, 0] == b, flat index = class * n + stored row,
// so equal scores go towards the lower (class, row) pair.  head is channel-major [c_total, n] (lvq_sparse_head's output).
__global__ __launch_bounds__(DEC_THREADS) void k_voxel_decode(const float *__restrict__ head, const int32_t *__restrict__ indices, int n_rows,
                                                               int n_tasks, CenterTasks tk, CenterGeom gm, int K, int box_dim,
                                                               float *__restrict__ boxes, float *__restrict__ scores,
                                                               int32_t *__restrict__ labels, int32_t *__restrict__ counts,
                                                               uint32_t *__restrict__ keys_ws, int64_t keys_pitch) {
    __shared__ SelectLds<DEC_THREADS, MAX_K> s;
    const int g = blockIdx.x, b = g / n_tasks, t = g - b * n_tasks, tid = threadIdx.x;
    const int n_cls = tk.n_cls[t];
    const float *hm = head + (int64_t)tk.off[t][5] * n_rows;
    // ---- the scene's row count n_b; K_eff = min(K, n_cls * n_b)
    if (tid == 0) s.ncand = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (int i = tid; i < n_rows; i += DEC_THREADS) mine += indices[3 * (int64_t)i] == b;
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d);
    if ((tid & 63) == 0 && mine) atomicAdd(&s.ncand, mine);
    __syncthreads();
    const int64_t cand = (int64_t)n_cls * s.ncand;
    const int k_eff = (int)(cand < K ? cand : K);
    __syncthreads();
    if (k_eff > 0)                                               // (workgroup-uniform)
        select_sort<DEC_THREADS, MAX_K, true>(s, [=](int i) {
            const int row = i % n_rows;
            return indices[3 * (int64_t)row] == b ? key_of(1.0f / (1.0f + expf(-hm[i]))) : 0u;
        }, keys_ws + (int64_t)g * keys_pitch, n_cls * n_rows, k_eff);
    decode_winners(s, k_eff, [&](uint32_t idx, int &cls, int &x, int &y) {
        cls = (int)(idx / (uint32_t)n_rows);
        const int row = (int)(idx - (uint32_t)cls * (uint32_t)n_rows);
        y = indices[3 * (int64_t)row + 1]; x = indices[3 * (int64_t)row + 2];
        return [=](int c) { return head[(int64_t)c * n_rows + row]; };
    }, tk, t, gm, g, K, box_dim, boxes, scores, labels, counts);
}

__global__ __launch_bounds__(256) void k_boxes_iou_bev(const float *__restrict__ a, int n, const float *__restrict__ bb, int m,
                                                        float *__restrict__ iou) {
    const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (i >= n || j >= m) return;
    iou[(int64_t)i * m + j] = rect_iou(rect_of(a + (int64_t)i * 7), rect_of(bb + (int64_t)j * 7));
}

__global__ __launch_bounds__(256) void k_center_collect(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                         const int32_t *__restrict__ labels, const int32_t *__restrict__ keep,
                                                         const int32_t *__restrict__ keep_count, int n_tasks, int k, int box_dim,
                                                         int post_max, float *__restrict__ out_boxes, float *__restrict__ out_scores,
                                                         int64_t *__restrict__ out_labels, int32_t *__restrict__ out_count) {
    __shared__ int start[MAX_TASKS + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        int s = 0;
        for (int t = 0; t < n_tasks; ++t) { start[t] = s; s += max(0, min(keep_count[b * n_tasks + t], post_max)); }
        start[n_tasks] = s;
        out_count[b] = s;
    }
    __syncthreads();
    const int64_t cap = (int64_t)n_tasks * post_max;
    for (int e = tid; e < (int)cap; e += 256) {
        const int t = e / post_max, j = e - t * post_max;
        const int g = b * n_tasks + t;
        if (j >= start[t + 1] - start[t]) continue;
        const int src = keep[(int64_t)g * post_max + j];
        if (src < 0 || src >= k) continue;                      // cannot happen behind lvq_nms_bev; never index with it
        const int64_t from = (int64_t)g * k + src, to = (int64_t)b * cap + start[t] + j;
        for (int d = 0; d < box_dim; ++d) out_boxes[to * box_dim + d] = boxes[from * box_dim + d];
        out_scores[to] = scores[from];
        out_labels[to] = (int64_t)labels[from] + 1;             // center_head.py:363: labels are 1-based
    }
}

// lvq_center_decode / lvq_voxel_decode: the ABI's host tables as CenterTasks and CenterGeom, with the refusals both entry points share, in
// their order.  cells >= 0: k may not exceed n_cls * cells in any task (the dense map's H * W; torch.topk raises there).
int center_tables(int n_tasks, const int32_t *task_channels, const int32_t *task_n_cls, const int32_t *class_map, int c_total, int k,
                  int box_dim, int stride, const float *voxel_xy, const float *range_xy, const float *limit_range, float score_thresh,
                  int64_t cells, CenterTasks &tk, CenterGeom &gm, int &max_cls) {
    if (n_tasks > MAX_TASKS) return LVQ_EUNSUPPORTED;
    tk = {};
    const int width[6] = {2, 1, 3, 2, 2, 0};
    int total_cls = 0;
    max_cls = 0;
    for (int t = 0; t < n_tasks; ++t) {
        const int nc = task_n_cls[t];
        if (nc <= 0) return LVQ_EINVAL;
        if (total_cls + nc > MAX_CLASSES) return LVQ_EUNSUPPORTED;
        if (cells >= 0 && (int64_t)k > (int64_t)nc * cells) return LVQ_EINVAL;
        for (int f = 0; f < 6; ++f) {
            const int c = task_channels[t * 6 + f], wd = f == 5 ? nc : width[f];
            if (f == 4 ? (box_dim == 9) != (c >= 0) : c < 0) return LVQ_EINVAL; // vel in every task of a 9-wide box, in none of a 7-wide one
            if (c >= 0 && c + wd > c_total) return LVQ_EINVAL;
            tk.off[t][f] = c;
        }
        tk.n_cls[t] = nc;
        tk.map_off[t] = total_cls;
        for (int c = 0; c < nc; ++c) tk.cls_map[total_cls + c] = class_map[total_cls + c];
        total_cls += nc;
        max_cls = nc > max_cls ? nc : max_cls;
    }
    if (k > MAX_K) return LVQ_EUNSUPPORTED;
    gm = center_geom(stride, voxel_xy, range_xy, limit_range, score_thresh);
    return LVQ_OK;
}

}  // namespace

extern "C" int lvq_center_decode_workspace_bytes(int batch, int n_tasks, int max_cls, int h, int w, size_t *bytes) {
    if (!bytes || batch <= 0 || n_tasks <= 0 || max_cls <= 0 || h <= 0 || w <= 0) return LVQ_EINVAL;
    const int64_t n = (int64_t)max_cls * h * w;
    if (n >= (1ll << 31) || n_tasks > MAX_TASKS || max_cls > MAX_CLASSES) return LVQ_EUNSUPPORTED;
    LvqSizer s;
    s.take<uint32_t>((size_t)batch * n_tasks * (size_t)lvq_align((size_t)n * 4, 256) / 4);
    *bytes = s.total();
    return LVQ_OK;
}

extern "C" int lvq_center_decode(const float *maps, int batch, int c_total, int h, int w, int n_tasks, const int32_t *task_channels,
                                 const int32_t *task_n_cls, const int32_t *class_map, int k, int box_dim, int stride,
                                 const float *voxel_xy, const float *range_xy, const float *limit_range, float score_thresh, float *boxes,
                                 float *scores, int32_t *labels, int32_t *counts, void *ws, size_t ws_bytes, lvq_stream_t stream) {
    if (!maps || !task_channels || !task_n_cls || !class_map || !voxel_xy || !range_xy || !limit_range || !boxes || !scores || !labels ||
        !counts || batch <= 0 || c_total <= 0 || h <= 0 || w <= 0 || n_tasks <= 0 || k <= 0 || stride <= 0 || (box_dim != 7 && box_dim != 9))
        return LVQ_EINVAL;
    CenterTasks tk;
    CenterGeom gm;
    int max_cls = 0;
    int rc = center_tables(n_tasks, task_channels, task_n_cls, class_map, c_total, k, box_dim, stride, voxel_xy, range_xy, limit_range,
                           score_thresh, (int64_t)h * w, tk, gm, max_cls);
    if (rc != LVQ_OK) return rc;
    size_t need = 0;
    rc = lvq_center_decode_workspace_bytes(batch, n_tasks, max_cls, h, w, &need);
    if (rc != LVQ_OK) return rc;
    if (!ws || ws_bytes < need) return LVQ_EWORKSPACE;
    const int64_t pitch = (int64_t)(lvq_align((size_t)max_cls * h * w * 4, 256) / 4);
    LvqArena arena(ws, ws_bytes);
    uint32_t *keys = arena.take<uint32_t>((size_t)batch * n_tasks * pitch);
    if (!arena.ok) return LVQ_EWORKSPACE;
    hipLaunchKernelGGL(k_center_decode, dim3((unsigned)(batch * n_tasks)), dim3(DEC_THREADS), 0, lvq_s(stream), maps, c_total, h, w, n_tasks, tk,
                       gm, k, box_dim, boxes, scores, labels, counts, keys, pitch);
    return lvq_launch_status();
}

extern "C" int lvq_voxel_decode_workspace_bytes(int batch, int n_tasks, int max_cls, int64_t n_rows, size_t *bytes) {
    if (!bytes || batch <= 0 || n_tasks <= 0 || max_cls <= 0 || n_rows < 0) return LVQ_EINVAL;
    const int64_t n = (int64_t)max_cls * n_rows;
    if (n >= (1ll << 31) || n_tasks > MAX_TASKS || max_cls > MAX_CLASSES) return LVQ_EUNSUPPORTED;
    LvqSizer s;
    s.take<uint32_t>((size_t)batch * n_tasks * (size_t)lvq_align((size_t)n * 4 + 4, 256) / 4);
    *bytes = s.total();
    return LVQ_OK;
}

extern "C" int lvq_voxel_decode(const float *head, const int32_t *indices, int64_t n_rows, int batch, int c_total, int n_tasks,
                                const int32_t *task_channels, const int32_t *task_n_cls, const int32_t *class_map, int k, int box_dim,
                                int stride, const float *voxel_xy, const float *range_xy, const float *limit_range, float score_thresh,
                                float *boxes, float *scores, int32_t *labels, int32_t *counts, void *ws, size_t ws_bytes, lvq_stream_t stream) {
    if (!task_channels || !task_n_cls || !class_map || !voxel_xy || !range_xy || !limit_range || !boxes || !scores || !labels || !counts ||
        batch <= 0 || c_total <= 0 || n_rows < 0 || n_tasks <= 0 || k <= 0 || stride <= 0 || (box_dim != 7 && box_dim != 9) ||
        (n_rows > 0 && (!head || !indices)))
        return LVQ_EINVAL;
    CenterTasks tk;
    CenterGeom gm;
    int max_cls = 0;
    int rc = center_tables(n_tasks, task_channels, task_n_cls, class_map, c_total, k, box_dim, stride, voxel_xy, range_xy, limit_range,
                           score_thresh, -1, tk, gm, max_cls);
    if (rc != LVQ_OK) return rc;
    size_t need = 0;
    rc = lvq_voxel_decode_workspace_bytes(batch, n_tasks, max_cls, n_rows, &need);
    if (rc != LVQ_OK) return rc;
    if (!ws || ws_bytes < need) return LVQ_EWORKSPACE;
    const int64_t pitch = (int64_t)(lvq_align((size_t)max_cls * n_rows * 4 + 4, 256) / 4);
    LvqArena arena(ws, ws_bytes);
    uint32_t *keys = arena.take<uint32_t>((size_t)batch * n_tasks * pitch);
    if (!arena.ok) return LVQ_EWORKSPACE;
    // (n_rows = 0: every group finds no candidate, reads no row and writes its zeros and its count)
    hipLaunchKernelGGL(k_voxel_decode, dim3((unsigned)(batch * n_tasks)), dim3(DEC_THREADS), 0, lvq_s(stream), head, indices, (int)n_rows, n_tasks,
                       tk, gm, k, box_dim, boxes, scores, labels, counts, keys, pitch);
    return lvq_launch_status();
}

extern "C" int lvq_boxes_iou_bev(const float *boxes_a, int n, const float *boxes_b, int m, float *iou, lvq_stream_t stream) {
    if (!boxes_a || !boxes_b || !iou || n <= 0 || m <= 0) return LVQ_EINVAL;
    if (lvq_cdiv(n, 4) > 65535) return LVQ_EUNSUPPORTED;
    hipLaunchKernelGGL(k_boxes_iou_bev, dim3((unsigned)lvq_cdiv(m, 64), (unsigned)lvq_cdiv(n, 4)), dim3(64, 4), 0, lvq_s(stream), boxes_a, n,
                       boxes_b, m, iou);
    return lvq_launch_status();
}

extern "C" int lvq_nms_bev_workspace_bytes(int groups, int n_max, size_t *bytes) {
    if (!bytes || groups <= 0 || n_max <= 0) return LVQ_EINVAL;
    if (n_max > MAX_K || groups > 65535) return LVQ_EUNSUPPORTED;
    LvqSizer s;
    s.take<uint64_t>((size_t)groups * n_max * nms_words(n_max));
    *bytes = s.total();
    return LVQ_OK;
}

extern "C" int lvq_nms_bev(const float *boxes, int box_stride, const int32_t *counts, int groups, int n_max, int pre_max, int post_max,
                           float thresh, int32_t *keep, int32_t *keep_count, void *ws, size_t ws_bytes, lvq_stream_t stream) {
    if (!boxes || !counts || !keep || !keep_count || groups <= 0 || n_max <= 0 || pre_max <= 0 || post_max <= 0 || box_stride < 7)
        return LVQ_EINVAL;
    size_t need = 0;
    const int rc = lvq_nms_bev_workspace_bytes(groups, n_max, &need);
    if (rc != LVQ_OK) return rc;
    if (!ws || ws_bytes < need) return LVQ_EWORKSPACE;
    return nms_launch<NMS_WORDS>(boxes, box_stride, counts, groups, n_max, pre_max, post_max, thresh, keep, keep_count, ws, ws_bytes, stream);
}

extern "C" int lvq_center_collect(const float *boxes, const float *scores, const int32_t *labels, const int32_t *keep,
                                  const int32_t *keep_count, int batch, int n_tasks, int k, int box_dim, int post_max, float *out_boxes,
                                  float *out_scores, int64_t *out_labels, int32_t *out_count, lvq_stream_t stream) {
    if (!boxes || !scores || !labels || !keep || !keep_count || !out_boxes || !out_scores || !out_labels || !out_count || batch <= 0 ||
        n_tasks <= 0 || k <= 0 || post_max <= 0 || (box_dim != 7 && box_dim != 9))
        return LVQ_EINVAL;
    if (n_tasks > MAX_TASKS || (int64_t)n_tasks * post_max >= (1ll << 31)) return LVQ_EUNSUPPORTED;
    hipLaunchKernelGGL(k_center_collect, dim3((unsigned)batch), dim3(256), 0, lvq_s(stream), boxes, scores, labels, keep, keep_count, n_tasks, k,
                       box_dim, post_max, out_boxes, out_scores, out_labels, out_count);
    return lvq_launch_status();
}
