// csrc/center_head.hip -- the post-processing of CenterHead (pcdet/models/dense_heads/center_head.py:297-365) for gfx950, wave64:
//
//   k_center_decode    centernet_utils.py:155-241.  One workgroup of 1024 threads per (scene, task): a 4 x 8-bit radix select of the K-th
//                      largest fp32 score over n_cls * H * W, a bitonic sort of the K winners in LDS, the box arithmetic, the masks and
//                      an order-keeping compaction.  Nothing is handed between workgroups.
//   k_voxel_decode     centernet_utils.py:243-354 (VoxelNeXtHead): the same selection, sort, masks and compaction (select_sort, decode_box, box_stays,
//                      compact_store are shared, not copied) over the ROWS of a sparse tensor: the candidates of a scene are the rows
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
// Every store below is an ordinary vector store from C++; LDS counters use ds atomics.
#include "common.h"

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
struct CenterGeom {
    float stride, vx, vy, rx, ry, lim[6], thresh;
};

// fp32 bits -> unsigned key with the order of the floats (negative values below positive ones).  Every NaN, whatever its sign bit and
// payload, gets the one top key: sigmoid(+NaN) carries the sign bit of -NaN through exp, the add and the divide, and would sort last.
__device__ __forceinline__ uint32_t key_of(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float score_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// LDS of the selection, shared by k_center_decode and k_voxel_decode
struct SelectLds {
    uint64_t buf[MAX_K];
    uint32_t hist[256], scan[2][256];
    uint32_t sel_bin, sel_above, sel_cnt, ncand;
    uint32_t wcnt[DEC_THREADS / 64];
};

// histogram of byte `shift` of the keys that agree with `prefix` above it.  Neighbouring candidates mostly fall into one bin, so a thread
// counts a run in a register and touches the LDS counter once per run.  key_at(i) is the key of flat index i, or 0 for an index that is
// no candidate (SPARSE only: key_of never returns 0, the lowest key is -inf's 0x007fffff).
template <bool FIRST, bool SPARSE, class KeyAt>
__device__ void radix_hist(KeyAt key_at, uint32_t *keys, int n, uint32_t prefix, int shift, uint32_t *hist) {
    int run_bin = -1;
    uint32_t run = 0;
    const uint32_t hi_mask = shift == 24 ? 0u : ~((1u << (shift + 8)) - 1u);
    for (int i = threadIdx.x; i < n; i += DEC_THREADS) {
        uint32_t k;
        if (FIRST) { k = key_at(i); keys[i] = k; }
        else k = keys[i];
        if (SPARSE && k == 0u) continue;
        if ((k & hi_mask) != prefix) continue;
        const int bin = (int)((k >> shift) & 255u);
        if (bin != run_bin) {
            if (run) atomicAdd(&hist[run_bin], run);
            run_bin = bin; run = 0;
        }
        ++run;
    }
    if (run) atomicAdd(&hist[run_bin], run);
}

// The K largest keys of key_at(0 .. n - 1), K >= 1 and at most the number of candidates, into s.buf[0 .. K - 1] as (key << 32 | ~index),
// descending: a 4 x 8-bit radix select of the K-th key, equal keys towards the lower flat index, then a bitonic sort.  keys [n] is the
// group's scratch in global memory.  Every thread of the workgroup calls it.
template <bool SPARSE, class KeyAt>
__device__ void select_sort(SelectLds &s, KeyAt key_at, uint32_t *keys, int n, int K) {
    uint64_t *buf = s.buf;
    uint32_t *hist = s.hist, *wcnt = s.wcnt;
    const int tid = threadIdx.x;
    // ---- the K-th largest key: four passes of 8 bits, most significant first
    uint32_t prefix = 0, need = (uint32_t)K;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        if (pass == 0) radix_hist<true, SPARSE>(key_at, keys, n, prefix, shift, hist);
        else radix_hist<false, SPARSE>(key_at, keys, n, prefix, shift, hist);
        __syncthreads();
        // suffix sums over the 256 bins (Hillis-Steele, 8 steps)
        if (tid < 256) s.scan[0][tid] = hist[tid];
        __syncthreads();
        int cur = 0;
        for (int d = 1; d < 256; d <<= 1) {
            if (tid < 256) s.scan[cur ^ 1][tid] = s.scan[cur][tid] + (tid + d < 256 ? s.scan[cur][tid + d] : 0u);
            __syncthreads();
            cur ^= 1;
        }
        if (tid < 256) {
            const uint32_t incl = s.scan[cur][tid], above = incl - hist[tid];
            if (above < need && incl >= need) { s.sel_bin = (uint32_t)tid; s.sel_above = above; s.sel_cnt = hist[tid]; }
        }
        __syncthreads();
        prefix |= s.sel_bin << shift;
        need -= s.sel_above;
        __syncthreads();
    }
    const uint32_t T = prefix, eq_cnt = s.sel_cnt;     // `need` of the eq_cnt keys equal to T belong to the K winners
    if (tid == 0) s.ncand = 0;
    __syncthreads();
    const bool all_equal = need == eq_cnt;
    for (int i = tid; i < n; i += DEC_THREADS) {
        const uint32_t k = keys[i];
        if (k > T || (all_equal && k == T)) {
            const uint32_t slot = atomicAdd(&s.ncand, 1u);
            if (slot < (uint32_t)MAX_K) buf[slot] = ((uint64_t)k << 32) | (uint64_t)(0xffffffffu - (uint32_t)i);
        }
    }
    if (!all_equal) {
        // more keys equal the K-th than there is room for: the lowest flat indices win.  Each thread owns a contiguous range.
        const int chunk = (n + DEC_THREADS - 1) / DEC_THREADS, lo = tid * chunk, hi = min(n, lo + chunk);
        uint32_t mine = 0;
        for (int i = lo; i < hi; ++i) mine += keys[i] == T;
        uint32_t before = 0;                                     // exclusive prefix: wave partials, then the waves before this one
        {
            const int lane = tid & 63, wave = tid >> 6;
            uint32_t v = mine;
            for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(v, d); if (lane >= d) v += o; }
            if (lane == 63) wcnt[wave] = v;
            __syncthreads();
            for (int q = 0; q < wave; ++q) before += wcnt[q];
            before += v - mine;
            __syncthreads();
        }
        for (int i = lo; i < hi && before < need; ++i)
            if (keys[i] == T) {
                const uint32_t slot = atomicAdd(&s.ncand, 1u);
                if (slot < (uint32_t)MAX_K) buf[slot] = ((uint64_t)T << 32) | (uint64_t)(0xffffffffu - (uint32_t)i);
                ++before;
            }
    }
    __syncthreads();
    // ---- sort the K winners: (key, ~index) descending, bitonic over the next power of two
    int P = 2;
    while (P < K) P <<= 1;
    if (tid < P && tid >= K) buf[tid] = 0;
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const int other = tid ^ j;
            if (tid < P && other > tid) {
                const uint64_t a = buf[tid], c = buf[other];
                const bool desc = (tid & k2) == 0;
                if (desc ? a < c : a > c) { buf[tid] = c; buf[other] = a; }
            }
            __syncthreads();
        }
}

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

// masks of centernet_utils.py:214-221 / 332-336
__device__ __forceinline__ bool box_stays(const float *bx, float sc, const CenterGeom &gm) {
    return bx[0] >= gm.lim[0] && bx[1] >= gm.lim[1] && bx[2] >= gm.lim[2] && bx[0] <= gm.lim[3] && bx[1] <= gm.lim[4] && bx[2] <= gm.lim[5] &&
           (gm.thresh < 0.f || sc > gm.thresh);
}

// order-keeping compaction of the kept candidates of group g (thread tid holds candidate tid) into rows g * K ..; rows behind the count
// are zeroed, counts[g] is written.  Every thread of the workgroup calls it.
__device__ void compact_store(uint32_t *wcnt, bool keep, const float *bx, float sc, int label, int g, int K, int box_dim,
                              float *__restrict__ boxes, float *__restrict__ scores, int32_t *__restrict__ labels, int32_t *__restrict__ counts) {
    const int tid = threadIdx.x;
    const uint64_t bal = __ballot(keep);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t rank = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)), total = 0;
    for (int q = 0; q < DEC_THREADS / 64; ++q) { const uint32_t c = wcnt[q]; total += c; if (q < wave) rank += c; }
    const int64_t row0 = (int64_t)g * K;
    if (keep) {
        for (int d = 0; d < box_dim; ++d) boxes[(row0 + rank) * box_dim + d] = bx[d];
        scores[row0 + rank] = sc;
        labels[row0 + rank] = label;
    }
    if (tid >= (int)total && tid < K) {                          // rows behind the count hold zeros, not what an earlier call left
        for (int d = 0; d < box_dim; ++d) boxes[(row0 + tid) * box_dim + d] = 0.f;
        scores[row0 + tid] = 0.f;
        labels[row0 + tid] = 0;
    }
    if (tid == 0) counts[g] = (int32_t)total;
}

__global__ __launch_bounds__(DEC_THREADS) void k_center_decode(const float *__restrict__ maps, int c_total, int h, int w, int n_tasks,
                                                                CenterTasks tk, CenterGeom gm, int K, int box_dim,
                                                                float *__restrict__ boxes, float *__restrict__ scores,
                                                                int32_t *__restrict__ labels, int32_t *__restrict__ counts,
                                                                uint32_t *__restrict__ keys_ws, int64_t keys_pitch) {
    __shared__ SelectLds s;
    const int g = blockIdx.x, b = g / n_tasks, t = g - b * n_tasks, tid = threadIdx.x;
    const int64_t hw = (int64_t)h * w;
    const int n = (int)(tk.n_cls[t] * hw);
    const float *scene = maps + (int64_t)b * c_total * hw;
    const float *hm = scene + (int64_t)tk.off[t][5] * hw;
    select_sort<false>(s, [hm](int i) { return key_of(1.0f / (1.0f + expf(-hm[i]))); }, keys_ws + (int64_t)g * keys_pitch, n, K);
    // ---- decode, mask, compact (centernet_utils.py:184-221)
    bool keep = false;
    float bx[9];
    float sc = 0.f;
    int label = 0;
    if (tid < K) {
        const uint64_t e = s.buf[tid];
        const uint32_t idx = 0xffffffffu - (uint32_t)(e & 0xffffffffu);
        sc = score_of((uint32_t)(e >> 32));
        const int cls = (int)(idx / (uint32_t)hw), pix = (int)(idx - (uint32_t)cls * (uint32_t)hw);
        const int y = pix / w, x = pix - y * w;
        decode_box([&](int c) { return scene[(int64_t)c * hw + pix]; }, x, y, tk.off[t], gm, box_dim, bx);
        keep = box_stays(bx, sc, gm);
        label = tk.cls_map[tk.map_off[t] + cls];
    }
    compact_store(s.wcnt, keep, bx, sc, label, g, K, box_dim, boxes, scores, labels, counts);
}

// centernet_utils.py:243-354 over rows: the candidates of scene b are the rows with indices[:, 0] == b, flat index = class * n + stored row,
// so equal scores go towards the lower (class, row) pair.  head is channel-major [c_total, n] (lvq_sparse_head's output).
__global__ __launch_bounds__(DEC_THREADS) void k_voxel_decode(const float *__restrict__ head, const int32_t *__restrict__ indices, int n_rows,
                                                               int n_tasks, CenterTasks tk, CenterGeom gm, int K, int box_dim,
                                                               float *__restrict__ boxes, float *__restrict__ scores,
                                                               int32_t *__restrict__ labels, int32_t *__restrict__ counts,
                                                               uint32_t *__restrict__ keys_ws, int64_t keys_pitch) {
    __shared__ SelectLds s;
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
        select_sort<true>(s, [=](int i) {
            const int row = i % n_rows;
            return indices[3 * (int64_t)row] == b ? key_of(1.0f / (1.0f + expf(-hm[i]))) : 0u;
        }, keys_ws + (int64_t)g * keys_pitch, n_cls * n_rows, k_eff);
    bool keep = false;
    float bx[9];
    float sc = 0.f;
    int label = 0;
    if (tid < k_eff) {
        const uint64_t e = s.buf[tid];
        const uint32_t idx = 0xffffffffu - (uint32_t)(e & 0xffffffffu);
        sc = score_of((uint32_t)(e >> 32));
        const int cls = (int)(idx / (uint32_t)n_rows), row = (int)(idx - (uint32_t)cls * (uint32_t)n_rows);
        const int y = indices[3 * (int64_t)row + 1], x = indices[3 * (int64_t)row + 2];
        decode_box([&](int c) { return head[(int64_t)c * n_rows + row]; }, x, y, tk.off[t], gm, box_dim, bx);
        keep = box_stays(bx, sc, gm);
        label = tk.cls_map[tk.map_off[t] + cls];
    }
    compact_store(s.wcnt, keep, bx, sc, label, g, K, box_dim, boxes, scores, labels, counts);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// rotated rectangles
// ---------------------------------------------------------------------------------------------------------------------------------
struct Rect { float x, y, hx, hy, c, s; };        // centre, half extents, cos / sin of the heading

__device__ __forceinline__ Rect rect_of(const float *p) {
    Rect r;
    r.x = p[0]; r.y = p[1]; r.hx = 0.5f * p[3]; r.hy = 0.5f * p[4];
    sincosf(p[6], &r.s, &r.c);
    return r;
}

// one Sutherland-Hodgman step against the half-plane sign * coord <= d, coord = x (AXIS 0) or y (AXIS 1); returns the new vertex count
template <int AXIS>
__device__ __forceinline__ int clip_plane(const float *px, const float *py, int n, float sign, float d, float *qx, float *qy) {
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 == n ? 0 : i + 1;
        const float vi = sign * (AXIS == 0 ? px[i] : py[i]) - d, vj = sign * (AXIS == 0 ? px[j] : py[j]) - d;
        const bool in_i = vi <= 0.f, in_j = vj <= 0.f;
        if (in_i && m < 8) { qx[m] = px[i]; qy[m] = py[i]; ++m; }
        if (in_i != in_j && m < 8) {
            const float tt = vi / (vi - vj);
            qx[m] = px[i] + tt * (px[j] - px[i]);
            qy[m] = py[i] + tt * (py[j] - py[i]);
            ++m;
        }
    }
    return m;
}

__device__ float rect_iou(const Rect &a, const Rect &b) {
    const float dx = a.x - b.x, dy = a.y - b.y;
    const float ra = a.hx + a.hy, rb = b.hx + b.hy;                       // >= the half diagonals
    if (dx * dx + dy * dy > (ra + rb) * (ra + rb)) return 0.f;            // the circumscribed circles are apart: the area is exactly zero
    const float ox = dx * b.c + dy * b.s, oy = dy * b.c - dx * b.s;       // a's centre in b's frame
    const float cr = a.c * b.c + a.s * b.s, sr = a.s * b.c - a.c * b.s;   // a's heading relative to b's
    const float ux = cr * a.hx, uy = sr * a.hx, vx = -sr * a.hy, vy = cr * a.hy;
    float px[8], py[8], qx[8], qy[8];
    px[0] = ox + ux + vx; py[0] = oy + uy + vy;
    px[1] = ox - ux + vx; py[1] = oy - uy + vy;
    px[2] = ox - ux - vx; py[2] = oy - uy - vy;
    px[3] = ox + ux - vx; py[3] = oy + uy - vy;
    int n = clip_plane<0>(px, py, 4, 1.f, b.hx, qx, qy);
    n = clip_plane<0>(qx, qy, n, -1.f, b.hx, px, py);
    n = clip_plane<1>(px, py, n, 1.f, b.hy, qx, qy);
    n = clip_plane<1>(qx, qy, n, -1.f, b.hy, px, py);
    float twice = 0.f;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 == n ? 0 : i + 1;
        twice += px[i] * py[j] - px[j] * py[i];
    }
    const float inter = 0.5f * fabsf(twice);
    const float sa = 4.f * a.hx * a.hy, sb = 4.f * b.hx * b.hy;
    return inter / fmaxf(sa + sb - inter, 1e-8f);
}

__global__ __launch_bounds__(256) void k_boxes_iou_bev(const float *__restrict__ a, int n, const float *__restrict__ bb, int m,
                                                        float *__restrict__ iou) {
    const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (i >= n || j >= m) return;
    iou[(int64_t)i * m + j] = rect_iou(rect_of(a + (int64_t)i * 7), rect_of(bb + (int64_t)j * 7));
}

__device__ __forceinline__ int group_count(const int32_t *counts, int g, int n_max, int pre_max) {
    return max(0, min(min(counts[g], n_max), pre_max));
}

__global__ __launch_bounds__(64) void k_nms_mask(const float *__restrict__ boxes, int box_stride, const int32_t *__restrict__ counts,
                                                  int n_max, int pre_max, float thresh, uint64_t *__restrict__ mask, int n_words) {
    __shared__ Rect rows[64];
    const int ct = blockIdx.x, rt = blockIdx.y, g = blockIdx.z, lane = threadIdx.x;
    if (ct < rt) return;                                        // strictly below the diagonal: a box is suppressed by EARLIER rows only
    const int n = group_count(counts, g, n_max, pre_max);
    if (ct * 64 >= n) return;                                   // the walk reads words 0 .. ceil(n / 64) - 1 of rows below n only
    const float *base = boxes + (int64_t)g * n_max * box_stride;
    const int col = ct * 64 + lane, row_l = rt * 64 + lane;
    Rect mine = {0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    if (col < n) mine = rect_of(base + (int64_t)col * box_stride);
    if (row_l < n) rows[lane] = rect_of(base + (int64_t)row_l * box_stride);
    __syncthreads();
    uint64_t word = 0;
    const int n_rows = min(64, n - rt * 64);
    for (int i = 0; i < n_rows; ++i) {
        const int row = rt * 64 + i;
        float v = 0.f;
        if (col < n && col > row) v = rect_iou(rows[i], mine);
        const uint64_t bal = __ballot(v > thresh);
        if (lane == i) word = bal;
    }
    if (row_l < n) mask[((int64_t)g * n_max + row_l) * n_words + ct] = word;
}

__global__ __launch_bounds__(64) void k_nms_walk(const uint64_t *__restrict__ mask, const int32_t *__restrict__ counts, int n_max,
                                                  int pre_max, int post_max, int n_words, int32_t *__restrict__ keep,
                                                  int32_t *__restrict__ keep_count) {
    __shared__ uint64_t tile[64][NMS_WORDS];
    const int g = blockIdx.x, lane = threadIdx.x;
    const int n = group_count(counts, g, n_max, pre_max);
    const uint64_t *gm = mask + (int64_t)g * n_max * n_words;
    int32_t *out = keep + (int64_t)g * post_max;
    uint64_t remv = 0;                                          // lane w holds word w of the removed set
    int cnt = 0;
    const int chunks = (n + 63) / 64;
    for (int c = 0; c < chunks && cnt < post_max; ++c) {
        const int rows_here = min(64, n - c * 64);
        // this chunk's rows, words c .. chunks - 1 (what k_nms_mask wrote), into LDS
        for (int e = lane; e < 64 * NMS_WORDS; e += 64) {
            const int r = e / NMS_WORDS, wd = e - r * NMS_WORDS;
            tile[r][wd] = (r < rows_here && wd >= c && wd < chunks) ? gm[(int64_t)(c * 64 + r) * n_words + wd] : 0ull;
        }
        __syncthreads();
        // the chunk's own decisions need the diagonal word alone: 64 uniform steps
        const uint64_t diag = tile[lane][c];
        const uint32_t d_lo = (uint32_t)diag, d_hi = (uint32_t)(diag >> 32);
        const uint32_t r_lo = (uint32_t)remv, r_hi = (uint32_t)(remv >> 32);
        uint64_t cur = ((uint64_t)(uint32_t)__shfl((int)r_hi, c) << 32) | (uint32_t)__shfl((int)r_lo, c);
        if (rows_here < 64) cur |= ~0ull << rows_here;
        uint64_t kept = 0;
        for (int j = 0; j < rows_here; ++j) {
            if ((cur >> j) & 1ull) continue;
            kept |= 1ull << j;
            cur |= ((uint64_t)(uint32_t)__shfl((int)d_hi, j) << 32) | (uint32_t)__shfl((int)d_lo, j);
        }
        // later words: lane w ORs the kept rows' word w
        if (lane > c && lane < chunks) {
            uint64_t k2 = kept;
            while (k2) {
                const int j = __ffsll((unsigned long long)k2) - 1;
                k2 &= k2 - 1;
                remv |= tile[j][lane];
            }
        }
        if ((kept >> lane) & 1ull) {
            const int pos = cnt + __popcll(kept & ((1ull << lane) - 1ull));
            if (pos < post_max) out[pos] = c * 64 + lane;
        }
        cnt += __popcll(kept);
        __syncthreads();
    }
    cnt = min(cnt, post_max);
    for (int e = cnt + lane; e < post_max; e += 64) out[e] = -1;
    if (lane == 0) keep_count[g] = cnt;
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

size_t nms_words(int n_max) { return (size_t)((n_max + 63) / 64); }

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
    if (n_tasks > MAX_TASKS) return LVQ_EUNSUPPORTED;
    CenterTasks tk = {};
    const int width[6] = {2, 1, 3, 2, 2, 0};
    int max_cls = 0, total_cls = 0;
    for (int t = 0; t < n_tasks; ++t) {
        const int nc = task_n_cls[t];
        if (nc <= 0) return LVQ_EINVAL;
        if (total_cls + nc > MAX_CLASSES) return LVQ_EUNSUPPORTED;
        if ((int64_t)k > (int64_t)nc * h * w) return LVQ_EINVAL;                 // torch.topk raises there
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
    size_t need = 0;
    const int rc = lvq_center_decode_workspace_bytes(batch, n_tasks, max_cls, h, w, &need);
    if (rc != LVQ_OK) return rc;
    if (!ws || ws_bytes < need) return LVQ_EWORKSPACE;
    CenterGeom gm;
    gm.stride = (float)stride; gm.vx = voxel_xy[0]; gm.vy = voxel_xy[1]; gm.rx = range_xy[0]; gm.ry = range_xy[1];
    for (int i = 0; i < 6; ++i) gm.lim[i] = limit_range[i];
    gm.thresh = score_thresh;
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
    if (n_tasks > MAX_TASKS) return LVQ_EUNSUPPORTED;
    CenterTasks tk = {};
    const int width[6] = {2, 1, 3, 2, 2, 0};
    int max_cls = 0, total_cls = 0;
    for (int t = 0; t < n_tasks; ++t) {
        const int nc = task_n_cls[t];
        if (nc <= 0) return LVQ_EINVAL;
        if (total_cls + nc > MAX_CLASSES) return LVQ_EUNSUPPORTED;
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
    size_t need = 0;
    const int rc = lvq_voxel_decode_workspace_bytes(batch, n_tasks, max_cls, n_rows, &need);
    if (rc != LVQ_OK) return rc;
    if (!ws || ws_bytes < need) return LVQ_EWORKSPACE;
    CenterGeom gm;
    gm.stride = (float)stride; gm.vx = voxel_xy[0]; gm.vy = voxel_xy[1]; gm.rx = range_xy[0]; gm.ry = range_xy[1];
    for (int i = 0; i < 6; ++i) gm.lim[i] = limit_range[i];
    gm.thresh = score_thresh;
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
    LvqArena arena(ws, ws_bytes);
    const int n_words = (int)nms_words(n_max);
    uint64_t *mask = arena.take<uint64_t>((size_t)groups * n_max * n_words);
    if (!arena.ok) return LVQ_EWORKSPACE;
    hipStream_t st = lvq_s(stream);
    hipLaunchKernelGGL(k_nms_mask, dim3((unsigned)n_words, (unsigned)n_words, (unsigned)groups), dim3(64), 0, st, boxes, box_stride, counts,
                       n_max, pre_max, thresh, mask, n_words);
    hipLaunchKernelGGL(k_nms_walk, dim3((unsigned)groups), dim3(64), 0, st, (const uint64_t *)mask, counts, n_max, pre_max, post_max, n_words,
                       keep, keep_count);
    return lvq_launch_status();
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
