// csrc/head_common.h -- what the dense heads' post-processing kernels share (center_head.hip, anchor_head.hip, transfusion_head.hip): the order of fp32
// scores as unsigned keys, the radix select + bitonic sort of the K best candidates, rotated rectangles and their IoU, the two
// kernels of the rotated BEV NMS, and for the heads that decode boxes on a grid (center_head.hip, transfusion_head.hip) the grid's
// geometry (CenterGeom), the range-and-threshold mask (box_stays) and the order-keeping compaction (compact_store).  Sizes are template
// parameters: THREADS is the workgroup's size, MAX_K the sort buffer's rows (a power of two), WORDS the 64-bit words of a row of the NMS
// mask that the walk keeps in LDS.  Everything sits in an anonymous namespace: each translation unit instantiates what it launches.
//
// Every store below is an ordinary vector store from C++; LDS counters use ds atomics.
#pragma once
#include "common.h"

namespace {

// fp32 bits -> unsigned key with the order of the floats (negative values below positive ones).  Every NaN, whatever its sign bit and
// payload, gets the one top key: sigmoid(+NaN) carries the sign bit of -NaN through exp, the add and the divide, and would sort last.
// -0.0 gets the key of +0.0 (0x80000000; its own, 0x7fffffff, stays unused): the two compare equal, in `score >= thresh` and in
// torch.topk, so between them the lower index decides, not the sign.  score_of turns that key back into +0.0.
__device__ __forceinline__ uint32_t key_of(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    if (u == 0x80000000u) return u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float score_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// LDS of the selection
template <int THREADS, int MAX_K>
struct SelectLds {
    uint64_t buf[MAX_K];
    uint32_t hist[256], scan[2][256];
    uint32_t sel_bin, sel_above, sel_cnt, ncand;
    uint32_t wcnt[THREADS / 64];
};

// histogram of byte `shift` of the words that agree with `prefix` above it.  Neighbouring candidates mostly fall into one bin, so a
// thread counts a run in a register and touches the LDS counter once per run.  word_at(i) is the word of position i, or 0 for a
// position that takes no part (SPARSE only: key_of never returns 0, the lowest key is -inf's 0x007fffff).
template <int THREADS, bool SPARSE, class WordAt>
__device__ void radix_hist(WordAt word_at, int n, uint32_t prefix, int shift, uint32_t *hist) {
    int run_bin = -1;
    uint32_t run = 0;
    const uint32_t hi_mask = shift == 24 ? 0u : ~((1u << (shift + 8)) - 1u);
    for (int i = threadIdx.x; i < n; i += THREADS) {
        const uint32_t k = word_at(i);
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

// The `need`-th largest of the words first(i) (pass 0) / later(i) (passes 1 .. 3; the same values), 1 <= need <= the number of words
// that take part: four passes of 8 bits, most significant first.  Returns the word; `need` becomes how many of the eq_cnt words equal to
// it belong to the winners.  Every thread of the workgroup calls it.
template <int THREADS, int MAX_K, bool SPARSE, class First, class Later>
__device__ uint32_t radix_kth(SelectLds<THREADS, MAX_K> &s, First first, Later later, int n, uint32_t &need, uint32_t &eq_cnt) {
    uint32_t *hist = s.hist;
    const int tid = threadIdx.x;
    uint32_t prefix = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        if (pass == 0) radix_hist<THREADS, SPARSE>(first, n, prefix, shift, hist);
        else radix_hist<THREADS, SPARSE>(later, n, prefix, shift, hist);
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
    eq_cnt = s.sel_cnt;
    return prefix;
}

// (key, ~index) words of s.buf[0 .. K - 1], descending: bitonic over the next power of two.  Every thread of the workgroup calls it.
template <int THREADS, int MAX_K>
__device__ void sort_desc(SelectLds<THREADS, MAX_K> &s, int K) {
    uint64_t *buf = s.buf;
    const int tid = threadIdx.x;
    int P = 2;
    while (P < K) P <<= 1;
    for (int i = tid; i < P; i += THREADS)
        if (i >= K) buf[i] = 0;
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += THREADS) {
                const int other = i ^ j;
                if (other > i) {
                    const uint64_t a = buf[i], c = buf[other];
                    const bool desc = (i & k2) == 0;
                    if (desc ? a < c : a > c) { buf[i] = c; buf[other] = a; }
                }
            }
            __syncthreads();
        }
}

// The K largest keys of key_at(0 .. n - 1), K >= 1 and at most the number of candidates, into s.buf[0 .. K - 1] as (key << 32 | ~index),
// descending: a 4 x 8-bit radix select of the K-th key, equal keys towards the lower flat index, then a bitonic sort.  keys [n] is the
// group's scratch in global memory.  Position i IS the flat index, so the plateau of keys equal to the K-th is cut by position: each
// thread owns a contiguous range.  Every thread of the workgroup calls it.
template <int THREADS, int MAX_K, bool SPARSE, class KeyAt>
__device__ void select_sort(SelectLds<THREADS, MAX_K> &s, KeyAt key_at, uint32_t *keys, int n, int K) {
    uint64_t *buf = s.buf;
    uint32_t *wcnt = s.wcnt;
    const int tid = threadIdx.x;
    uint32_t need = (uint32_t)K, eq_cnt = 0;
    const uint32_t T = radix_kth<THREADS, MAX_K, SPARSE>(s, [&](int i) { const uint32_t k = key_at(i); keys[i] = k; return k; },
                                                          [&](int i) { return keys[i]; }, n, need, eq_cnt);
    // `need` of the eq_cnt keys equal to T belong to the K winners
    if (tid == 0) s.ncand = 0;
    __syncthreads();
    const bool all_equal = need == eq_cnt;
    for (int i = tid; i < n; i += THREADS) {
        const uint32_t k = keys[i];
        if (k > T || (all_equal && k == T)) {
            const uint32_t slot = atomicAdd(&s.ncand, 1u);
            if (slot < (uint32_t)MAX_K) buf[slot] = ((uint64_t)k << 32) | (uint64_t)(0xffffffffu - (uint32_t)i);
        }
    }
    if (!all_equal) {
        // more keys equal the K-th than there is room for: the lowest flat indices win.  Each thread owns a contiguous range.
        const int chunk = (n + THREADS - 1) / THREADS, lo = tid * chunk, hi = min(n, lo + chunk);
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
    sort_desc(s, K);
}

// select_sort for candidates that come in NO PARTICULAR ORDER: position i names the flat index index_at(i) (all different).  The
// plateau of keys equal to the K-th is cut by a second radix select, over ~index among those keys, so the winners -- equal keys
// towards the lower flat index -- do not depend on the positions.  keys [n] as above.  Every thread of the workgroup calls it.
template <int THREADS, int MAX_K, bool SPARSE, class KeyAt, class IndexAt>
__device__ void select_sort_unordered(SelectLds<THREADS, MAX_K> &s, KeyAt key_at, IndexAt index_at, uint32_t *keys, int n, int K) {
    uint64_t *buf = s.buf;
    const int tid = threadIdx.x;
    uint32_t need = (uint32_t)K, eq_cnt = 0;
    const uint32_t T = radix_kth<THREADS, MAX_K, SPARSE>(s, [&](int i) { const uint32_t k = key_at(i); keys[i] = k; return k; },
                                                          [&](int i) { return keys[i]; }, n, need, eq_cnt);
    uint32_t T2 = 0;                                             // every ~index of a key equal to T is at least T2 ...
    if (need != eq_cnt) {                                        // ... unless the plateau has to be cut (workgroup-uniform)
        // ~index is never 0 for an index below 2^31, so 0 can stand for "takes no part"
        auto inv = [&](int i) { return keys[i] == T ? 0xffffffffu - (uint32_t)index_at(i) : 0u; };
        uint32_t need2 = need, eq2 = 0;
        T2 = radix_kth<THREADS, MAX_K, true>(s, inv, inv, n, need2, eq2);
    }
    if (tid == 0) s.ncand = 0;
    __syncthreads();
    for (int i = tid; i < n; i += THREADS) {
        const uint32_t k = keys[i];
        if (SPARSE && k == 0u) continue;
        const uint32_t ni = 0xffffffffu - (uint32_t)index_at(i);
        if (k > T || (k == T && ni >= T2)) {
            const uint32_t slot = atomicAdd(&s.ncand, 1u);
            if (slot < (uint32_t)MAX_K) buf[slot] = ((uint64_t)k << 32) | (uint64_t)ni;
        }
    }
    __syncthreads();
    sort_desc(s, K);
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

// ---------------------------------------------------------------------------------------------------------------------------------
// rotated BEV NMS: the suppression words, then the walk
// ---------------------------------------------------------------------------------------------------------------------------------
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

// One wave per group walks the rows on the device.  WORDS >= n_words: lane w holds word w of the removed set, so 64 words -- 4096
// rows -- are the most a wave can walk.
template <int WORDS>
__global__ __launch_bounds__(64) void k_nms_walk(const uint64_t *__restrict__ mask, const int32_t *__restrict__ counts, int n_max,
                                                  int pre_max, int post_max, int n_words, int32_t *__restrict__ keep,
                                                  int32_t *__restrict__ keep_count) {
    __shared__ uint64_t tile[64][WORDS];
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
        for (int e = lane; e < 64 * WORDS; e += 64) {
            const int r = e / WORDS, wd = e - r * WORDS;
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

// ---------------------------------------------------------------------------------------------------------------------------------
// decoded boxes: the geometry of the grid, the range-and-threshold mask, the order-keeping compaction
// ---------------------------------------------------------------------------------------------------------------------------------
struct CenterGeom {                    // by value in the kernel arguments
    float stride, vx, vy, rx, ry, lim[6], thresh;
};

inline CenterGeom center_geom(int stride, const float *voxel_xy, const float *range_xy, const float *limit_range, float score_thresh) {
    CenterGeom gm;
    gm.stride = (float)stride; gm.vx = voxel_xy[0]; gm.vy = voxel_xy[1]; gm.rx = range_xy[0]; gm.ry = range_xy[1];
    for (int i = 0; i < 6; ++i) gm.lim[i] = limit_range[i];
    gm.thresh = score_thresh;
    return gm;
}

// the centre inside the limit range and the score above the threshold (centernet_utils.py:214-221 / 332-336, transfusion_head.py:433-451).
// THRESH_OPTIONAL: a negative threshold stands for "none" and keeps every score (the centre heads' SCORE_THRESH None); without it the
// threshold is applied whatever its sign (TransFusionHead).
template <bool THRESH_OPTIONAL>
__device__ __forceinline__ bool box_stays(const float *bx, float sc, const CenterGeom &gm) {
    return bx[0] >= gm.lim[0] && bx[1] >= gm.lim[1] && bx[2] >= gm.lim[2] && bx[0] <= gm.lim[3] && bx[1] <= gm.lim[4] && bx[2] <= gm.lim[5] &&
           ((THRESH_OPTIONAL && gm.thresh < 0.f) || sc > gm.thresh);
}

// order-keeping compaction of the kept candidates of group g (thread tid holds candidate tid) into rows g * K ..; rows behind the count
// are zeroed, counts[g] is written.  wcnt: THREADS / 64 LDS words.  Every thread of the workgroup (THREADS of them) calls it.
template <int THREADS>
__device__ void compact_store(uint32_t *wcnt, bool keep, const float *bx, float sc, int label, int g, int K, int box_dim,
                              float *__restrict__ boxes, float *__restrict__ scores, int32_t *__restrict__ labels, int32_t *__restrict__ counts) {
    const int tid = threadIdx.x;
    const uint64_t bal = __ballot(keep);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t rank = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)), total = 0;
    for (int q = 0; q < THREADS / 64; ++q) { const uint32_t c = wcnt[q]; total += c; if (q < wave) rank += c; }
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

inline size_t nms_words(int n_max) { return (size_t)((n_max + 63) / 64); }

// the shared body of lvq_nms_bev / lvq_nms_bev_wide: n_max <= 64 * WORDS is the caller's check
template <int WORDS>
int nms_launch(const float *boxes, int box_stride, const int32_t *counts, int groups, int n_max, int pre_max, int post_max, float thresh,
               int32_t *keep, int32_t *keep_count, void *ws, size_t ws_bytes, lvq_stream_t stream) {
    LvqArena arena(ws, ws_bytes);
    const int n_words = (int)nms_words(n_max);
    uint64_t *mask = arena.take<uint64_t>((size_t)groups * n_max * n_words);
    if (!arena.ok) return LVQ_EWORKSPACE;
    hipStream_t st = lvq_s(stream);
    hipLaunchKernelGGL(k_nms_mask, dim3((unsigned)n_words, (unsigned)n_words, (unsigned)groups), dim3(64), 0, st, boxes, box_stride, counts,
                       n_max, pre_max, thresh, mask, n_words);
    hipLaunchKernelGGL(k_nms_walk<WORDS>, dim3((unsigned)groups), dim3(64), 0, st, (const uint64_t *)mask, counts, n_max, pre_max, post_max,
                       n_words, keep, keep_count);
    return lvq_launch_status();
}

}  // namespace
