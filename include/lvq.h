/*
 * include/lvq.h -- C ABI of liblvq_hip.so, the MI355X (gfx950) implementation of the LiDAR-vision
 * fusion hot path of Advaith-Sajeev/LiDAR-Vision-VQA.
 *
 * The reference has NO FFI on this path: its boundary is Python nn.Module / numpy duck-typing
 * (SURVEY.md 8b).  Each entry point below therefore names the reference Python interface whose
 * arithmetic it replaces (file:line relative to /root/reference/src/); the Python host side in
 * lidar-vision-vqa_amd/{lidar,fusion,head}/ mirrors those interfaces 1:1 and binds these symbols
 * through ctypes (lidar-vision-vqa_amd/_ffi.py).  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions (all functions):
 *   - extern "C", plain pointers and sizes, no torch / HIP types in the signatures
 *     (`lvq_stream_t` is a hipStream_t passed as void*; NULL = the null stream).
 *   - every pointer is a DEVICE pointer unless the parameter comment says "host".
 *   - the caller owns every buffer, including the workspace whose size is queried first;
 *     nothing is allocated, freed or synchronised inside a call -> stream-ordered, asynchronous,
 *     graph-capturable, thread-safe per stream.  The library never reads the environment; its only process-wide state is the
 *     tuning record below (kernel-family choices and test hooks), which the caller sets explicitly (lvq_set_tuning) and which
 *     changes speed or the kernel family, never results beyond what each field documents.
 *   - return value: LVQ_OK (0) or a negative LVQ_E* code; never throws, never exits.
 *   - rows are contiguous, row-major; "bf16" is the upper 16 bits of an IEEE fp32 (uint16_t).
 */
#ifndef LVQ_H
#define LVQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *lvq_stream_t;
typedef uint16_t lvq_bf16;

enum {
    LVQ_OK = 0,
    LVQ_EINVAL = -1,      /* bad argument (null pointer, non-positive size, unsupported combination) */
    LVQ_EWORKSPACE = -2,  /* workspace too small */
    LVQ_ELAUNCH = -3,     /* hipLaunch / runtime error (hipGetLastError != success) */
    LVQ_EOVERFLOW = -4,   /* key space does not fit (e.g. batch * grid cells >= 2^31, see lvq_voxelize_dynamic) */
    LVQ_EUNSUPPORTED = -5 /* shape outside what the kernels implement (documented per function) */
};

const char *lvq_version(void);
const char *lvq_strerror(int code);

/* Kernel-family choices that are not implied by the shapes: every routing decision that used to hide behind a getenv inside the library
 * (VERDICT r2).  All zeros = the built-in choices (lvq_tuning_defaults).  Process-wide: set it before launching, not concurrently with
 * launches of other threads.  The Python mirror fills it from the LVQ_* environment variables of INTEGRATION.md (lidar-vision-vqa_amd/_ffi.py);
 * all variants of one entry point are held to the same oracle by the tests (for lvq_gemm_bf16 and lvq_attention_bf16:
 * tests/test_gpu_kernel_routes.py, every field below that routes them against fp64). */
typedef struct lvq_tuning {
    int32_t attn_no32;               /* 1: the 16x16x32 attention kernel for long K/V streams instead of k_attn32 */
    int32_t attn32_nw;               /* k_attn32 waves per workgroup: 0 auto, 4 or 6 */
    int32_t attn_pipe;               /* k_attn32 with 4 waves: 0 auto (pipelined for hi + lo / fp16 queries), 1 always pipelined, -1 never */
    int32_t attn_nsplit;             /* KV split count of the attention kernels: 0 auto, 1..64 (test hook: 1 = direct output path) */
    int32_t attn_qt;                 /* k_attn query tiles per wave: 0 auto, 1 or 2 (other values are ignored) */
    int32_t attn_nw;                 /* k_attn waves per workgroup: 0 auto, 4, 8 or 12 */
    int32_t gemm_no_gemv;            /* 1: MFMA tile kernels also for M <= 8 (instead of the skinny-M GEMV) */
    int32_t gemm_stream_c_mb;        /* output size (MB) from which GEMM outputs use non-temporal stores: 0 = 32, -1 = never */
    int32_t gemm_no256;              /* 1: no 8-wave 256x128 / 256x256 GEMM kernels (128x128 tiles) */
    int32_t gemm_no256x256;          /* 1: no 256x256 GEMM kernel */
    int32_t gemm_256x256_min_tiles;  /* tile count from which the 256x256 kernel is used: 0 = 1024 or one full dispatch round */
    int32_t gemm_ln_tiles;           /* 1: tile kernel instead of the row-streaming Linear + LayerNorm kernel */
    int32_t pillar_vfe_generic;      /* 1: generic multi-layer PillarVFE kernel instead of the single-layer one */
    int32_t voxel_path;              /* hard / dynamic voxeliser: 0 default (hash-balanced slabs / slab-binned), 1 slab-binned, 2 global hash / two-level bitmap */
    int32_t pairs_one_wg;            /* 1: lvq_bev_scene_pairs with one workgroup per scene */
    int32_t ca_fused_variant;        /* diagnostics builds (CA_DEBUG_VARIANTS) only: timing-ablation variant of k_ca_fused; results are wrong */
    uint64_t ca_fused_stamps;        /* diagnostics: device pointer to [workgroups][4][8] uint64 that k_ca_fused fills with s_memrealtime stamps, or 0 */
    int32_t conv_rows_grid;          /* test hook: workgroups of k_conv_rows (two-launch lvq_bev_tile_kv): 0 built-in grid, n > 0 at most n */
    int32_t pillar_vfe_path;         /* single-layer PillarVFE kernel: 0 packed (live points of several pillars per MFMA tile), 1 one pillar per wave; same bits */
    int32_t reserved[6];
} lvq_tuning;
void lvq_tuning_defaults(lvq_tuning *t);
int lvq_set_tuning(const lvq_tuning *t);      /* NULL restores the defaults */
int lvq_get_tuning(lvq_tuning *t);

/* =====================================================================================
 * LiDAR side
 * ===================================================================================== */

/* a1  pcdet/utils/common_utils.py:78-81 mask_points_by_range (via data_processor.py:79-93):
 * keep[i] = lo_x <= x <= hi_x && lo_y <= y <= hi_y  (INCLUSIVE, z untested).
 * pts [n,c] fp32 (x,y in columns 0,1); keep [n] uint8; range: host float[6]. */
int lvq_mask_points_by_range(const float *pts, int64_t n, int c, const float *range_host, uint8_t *keep,
                             lvq_stream_t stream);

/* a3  data_processor.py:16-61,133-180  VoxelGeneratorWrapper.generate -> spconv Point2VoxelCPU3d
 * (hard voxelisation), batched over scenes so that collate_batch (dataset.py:230-244, a4) is fused:
 * outputs are the CONCATENATED per-scene results with the batch index already prepended.
 *   pts            [n_points, c] fp32, scenes stored back to back; columns 0..2 = x,y,z
 *   scene_off      [n_scenes+1] int32 point offsets (scene s owns points scene_off[s]..scene_off[s+1])
 *   range/vsize/grid  host float[6] / float[3] / int32[3] (nx,ny,nz)
 *   max_pts        T = MAX_POINTS_PER_VOXEL;   max_voxels = per-scene cap
 *   break_on_cap   0 = spconv>=1.1/2.x `continue` semantics (default), 1 = spconv-1.0 `break`
 *   voxel_capacity rows available in the three outputs; must be >= min(n_points, n_scenes*max_voxels)
 *   voxels         [cap, T, c] fp32  (zero padded)
 *   coords_bzyx    [cap, 4] int32    (batch, z, y, x)
 *   num_pts        [cap] int32
 *   scene_voxel_off[n_scenes+1] int32: scene s owns output rows [off[s], off[s+1]); off[n_scenes] = total M
 * Voxel order inside a scene = first appearance in input order; the first T points of a voxel in
 * input order are kept: bit-exact with the sequential CPU algorithm. */
size_t lvq_voxelize_hard_workspace_bytes(int64_t n_points, int n_scenes);
int lvq_voxelize_hard(const float *pts, const int32_t *scene_off, int64_t n_points, int n_scenes, int c,
                      const float *range_host, const float *vsize_host, const int32_t *grid_host,
                      int max_pts, int max_voxels, int break_on_cap, int64_t voxel_capacity,
                      float *voxels, int32_t *coords_bzyx, int32_t *num_pts, int32_t *scene_voxel_off,
                      void *ws, size_t ws_bytes, lvq_stream_t stream);

/* a3 + a5 fused ("fused voxelise -> mean", 16 N + M (4 C + 16) bytes, no padded [M,T,C] tensor):
 * the voxelisation of lvq_voxelize_hard (`continue` cap) whose per-voxel payload is MeanVFE's row
 * (mean_vfe.py:25-29): voxel_features[m,:] = sum of the first min(count, T) points in input order / that count --
 * the same fp32 additions in the same order as lvq_voxelize_hard + lvq_mean_vfe, hence bit-identical to that pair.
 * coords / num_pts / scene_voxel_off / workspace (lvq_voxelize_hard_workspace_bytes) as for lvq_voxelize_hard.
 * c == 4, T <= 127, key space < 2^31, N <= 4 M, <= 1024 scenes; otherwise LVQ_EUNSUPPORTED (run the pair instead). */
int lvq_voxelize_mean(const float *pts, const int32_t *scene_off, int64_t n_points, int n_scenes, int c,
                      const float *range_host, const float *vsize_host, const int32_t *grid_host, int max_pts,
                      int max_voxels, int64_t voxel_capacity, float *voxel_features, int32_t *coords_bzyx,
                      int32_t *num_pts, int32_t *scene_voxel_off, void *ws, size_t ws_bytes, lvq_stream_t stream);

/* a5  backbones_3d/vfe/mean_vfe.py:25-29  MeanVFE.forward:
 * out[m,:] = sum_t voxels[m,t,:] / max(num_pts[m],1).  n_voxels_dev (optional, may be NULL) points at
 * a device int32 holding the live row count (<= m_cap), so the call needs no host sync. */
int lvq_mean_vfe(const float *voxels, const int32_t *num_pts, int64_t m_cap, const int32_t *n_voxels_dev,
                 int t, int c, float *out, lvq_stream_t stream);

/* a6  backbones_3d/vfe/pillar_vfe.py:8-49,94-123  PillarVFE.forward + PFNLayer (eval BatchNorm folded
 * into scale/shift by the caller: scale = gamma/sqrt(var+eps), shift = beta - mean*scale; with
 * USE_NORM=False pass scale=1, shift=linear.bias).
 *   voxels [m,T,c], num_pts [m], coords_bzyx [m,4]
 *   n_layers PFN layers; layer l has weight w[l] [cout_l, cin_l] fp32 and scale/shift [cout_l];
 *   w/scale/shift: HOST arrays of n_layers DEVICE pointers; cin/cout: host int arrays.
 *   flags bit0 = USE_ABSLOTE_XYZ, bit1 = WITH_DISTANCE
 *   voxel geometry: vsize[3], offset[3] = vsize/2 + range_lo  (host)
 *   out [m, cout_last] fp32; rows >= *n_voxels_dev (if given) are not written.
 *   Shape rule.  LVQ_EINVAL: t <= 0, c < 3, n_layers < 1, cin_0 != (bit0 ? c : c - 3) + 6 + (bit1 ? 1 : 0), or
 *   cin_l != 2 cout_{l-1} for l >= 1 (a non-final layer hands [x, x_max] on).  LVQ_EUNSUPPORTED: n_layers > 4, T > 64, a
 *   cout_l > 256 or cin_l > 512, or T * cmax > 20480 with cmax = max(c, every cin_l, 2 cout_l of the non-final layers,
 *   cout of the last): one wave keeps two [T][cmax] fp32 planes in LDS, and the workgroup shrinks from 4 waves to 2 to 1
 *   until they fit in 160 KB.  So every T <= 40 runs at any width the other limits allow, T = 64 up to cmax = 320
 *   (e.g. [64, 64] and [160, 256]), and T = 32 with cout = 256.  Nothing is written when a call is refused.
 *   Kernels.  One layer, c = 4, T <= 32, cin <= 12, cout <= 64 and voxels on a 16-byte boundary take the single-layer path:
 *   by default the packed kernel (two pillars per wave pass, the live points of several pillars per f32 MFMA tile), with
 *   lvq_tuning.pillar_vfe_path = 1 the one-pillar-per-wave kernel; the two return the same bits.  Everything else, and every
 *   call under lvq_tuning.pillar_vfe_generic = 1, takes the generic multi-layer kernel (sequential mean: same bound, other bits). */
int lvq_pillar_vfe(const float *voxels, const int32_t *num_pts, const int32_t *coords_bzyx, int64_t m_cap,
                   const int32_t *n_voxels_dev, int t, int c, int n_layers, const float *const *w_host,
                   const float *const *scale_host, const float *const *shift_host, const int32_t *cin_host,
                   const int32_t *cout_host, int flags, const float *vsize_host, const float *offset_host,
                   float *out, lvq_stream_t stream);

/* a7  backbones_3d/vfe/dynamic_mean_vfe.py:53-64, dynamic_pillar_vfe.py:93-103,
 *     dynamic_voxel_vfe.py:60-71: floor((xyz-lo)/vs).int(), range mask, int32 linear key,
 *     torch.unique(sorted, return_inverse, return_counts), key decode -> (b,z,y,x).
 *   pts        [n, c] fp32, column 0 = batch index, 1..3 = x,y,z   (c >= 4)
 *   ndim       3: key = b*nx*ny*nz + cx*ny*nz + cy*nz + cz ; 2: key = b*nx*ny + cx*ny + cy (z untested)
 *   batch_size number of scenes (keys must stay below 2^31: else LVQ_EOVERFLOW -- the reference
 *              silently wraps int32 there; that quirk is NOT reproduced)
 *   unq_inv    [n] int32: rank of the point's voxel among the unique keys (ascending = torch.unique
 *              order), -1 for points outside the grid (the reference drops them)
 *   pt_coords  [n,3] int32 (cx,cy,cz) or NULL
 *   unq_key    [cap] int32, unq_cnt [cap] int32, coords_bzyx [cap,4] int32,  cap >= min(n, key space)
 *   counts     [2] int32: counts[0] = M unique voxels, counts[1] = N' valid points */
size_t lvq_voxelize_dynamic_workspace_bytes(int64_t n_points, int batch_size, const int32_t *grid_host, int ndim);
int lvq_voxelize_dynamic(const float *pts, int64_t n, int c, int batch_size, const float *range_host,
                         const float *vsize_host, const int32_t *grid_host, int ndim, int32_t *unq_inv,
                         int32_t *pt_coords, int32_t *unq_key, int32_t *unq_cnt, int32_t *coords_bzyx,
                         int32_t *counts, void *ws, size_t ws_bytes, lvq_stream_t stream);

/* lvq_voxel_slab_plan (host only, a hook for tests): how the slab-binned kernels (csrc/voxel_binned.hip) would cut a key space --
 * the ranking step behind lvq_voxelize_dynamic (dynamic_mean_vfe.py:53-72), lvq_voxelize_hard with voxel_path 1,
 * lvq_sparse_conv_rules and lvq_sparse_bev_merge.  Slab s holds the keys [s << *logslab, (s + 1) << *logslab); one workgroup ranks it.
 *   keyspace   batch * grid cells (the dynamic entry's key space: 2-D or 3-D; the rule builder's: batch * output cells)
 *   n          points, or candidate cells (lvq_sparse_conv_rules: n_in * prod(ceil(k / s)); n_in for submanifold layers)
 *   hard       0: the dynamic kernels (slabs up to 2^18 keys), 1: the hard kernels (up to 2^17)
 *   caps       HOST int[4], the constants the slab kernels branch on: [0] voxels of a slab whose counters the dynamic write kernel
 *              keeps in LDS, [1] voxels and [2] points of a slab whose state the hard slab kernel keeps in LDS (more: global
 *              stand-ins), [3] points up to which a slab takes the hard path's brute-force kernel
 * Launches nothing and touches no device memory.  NULL output, keyspace <= 0, n < 0 or hard outside {0, 1}: LVQ_EINVAL; a key space of
 * 2^31 or more: LVQ_EOVERFLOW; one the binned kernels do not take (the caller's next path runs): LVQ_EUNSUPPORTED. */
int lvq_voxel_slab_plan(int64_t keyspace, int64_t n, int hard, int *logslab, int *nslabs, int *caps);

/* torch_scatter.scatter_mean(points[:,col0:col0+nc], unq_inv) as used by DynamicMeanVFE
 * (dynamic_mean_vfe.py:64) and for points_mean in the PFN variants (dynamic_pillar_vfe.py:105).
 * sums [m_cap,nc] must be zero on entry; on exit out = sums / max(cnt,1) (out may alias sums). */
int lvq_scatter_mean(const float *pts, int64_t n, int c, int col0, int nc, const int32_t *unq_inv,
                     const int32_t *unq_cnt, int64_t m_cap, float *sums, float *out, lvq_stream_t stream);

/* a7  DynamicPillarVFE / DynamicVoxelVFE / DynamicPillarVFESimple2D forward after the unique step
 * (dynamic_pillar_vfe.py:105-127,210-227; dynamic_voxel_vfe.py:73-92) with PFNLayerV2
 * (dynamic_pillar_vfe.py:35-46), BatchNorm folded as in lvq_pillar_vfe.
 *   kind 0 = pillar (f_center z = z - z_offset), 1 = voxel (per-cell z centre), 2 = simple2d (no f_cluster)
 *   points_mean [m,3] from lvq_scatter_mean (ignored for kind 2)
 *   n_layers <= 2, cout_l <= 256, at most 16 augmented features (cin_0 = (bit0 ? c - 1 : c - 4) + (kind 2 ? 3 : 6) +
 *   (bit1 ? 1 : 0)): otherwise LVQ_EUNSUPPORTED; a cin_0 other than that count or cin_1 != 2 cout_0: LVQ_EINVAL.
 *   xmax_tmp [m_cap, cout_0] scratch for 2-layer nets (zero on entry), out [m_cap, cout_last] zero on entry (post-ReLU
 *   maxima are >= 0; a voxel that receives no point keeps its zero). */
int lvq_dynamic_pfn(const float *pts, int64_t n, int c, const int32_t *unq_inv, const int32_t *pt_coords,
                    const float *points_mean, int kind, int n_layers, const float *const *w_host,
                    const float *const *scale_host, const float *const *shift_host, const int32_t *cin_host,
                    const int32_t *cout_host, int flags, const float *vsize_host, const float *offset_host,
                    float *xmax_tmp, float *out, lvq_stream_t stream);

/* a8  backbones_2d/map_to_bev/pointpillar_scatter.py:14-37  PointPillarScatter.forward:
 * canvas[b, ch, y, x] = feat[m, ch] for coords (b, z, y, x) with nz == 1; canvas is zero-filled here. */
int lvq_pillar_scatter(const float *feat, const int32_t *coords_bzyx, int64_t m_cap, const int32_t *n_voxels_dev,
                       int ch, int batch, int ny, int nx, float *canvas, lvq_stream_t stream);

/* =====================================================================================
 * Fusion side (VATBlock / VATLiDAR / VATVision / VisionAdapter building blocks)
 * ===================================================================================== */

/* Precision modes of the fusion kernels.  Accumulation, LayerNorm / softmax statistics and residuals
 * are always fp32.  Every bf16 tensor may travel as ONE array (plain bf16 operands, "bf16") or as a
 * hi + lo PAIR (x = hi + lo to ~2^-17, "bf16x3": products are formed as hi*hi + hi*lo + lo*hi on the same
 * bf16 MFMA tiles).  Passing the `_lo` pointers selects the mode per call; producers write the lo twin
 * when its pointer is non-NULL.  bf16x3 is the mode that meets the 1e-3 parity bar against the fp32 CPU
 * path (plain bf16 operand rounding alone is ~2e-3 of max|out|; see DESIGN.md "Numerics"). */

/* nn.LayerNorm over the last dim (eps 1e-5 in every reference use: vat_blocks.py:19,23,27,
 * vat_lidar.py:89,114,116, vision_adapter.py:56).  x [rows,d] fp32 (+ optional per-row-group
 * additive embedding: x[r,:] + add[(r / add_group) % add_rows, :] BEFORE the norm -- VisionAdapter's
 * `t + view_embed[v]`, vision_adapter.py:122) and an optional table added AFTER the norm,
 * y[r,:] += post_add[r % post_rows, :] (VATLiDAR's cached geo_pe + view_embed[sid], vat_lidar.py:235-248).
 * Writes y_f32 and/or y_bf16 (+ y_lo). */
int lvq_layernorm(const float *x, const float *add, int add_rows, int add_group, const float *gamma,
                  const float *beta, float eps, int64_t rows, int d, const float *post_add, int64_t post_rows,
                  float *y_f32, lvq_bf16 *y_bf16, lvq_bf16 *y_lo, lvq_stream_t stream);

/* Linear layer on MFMA bf16 tiles with fp32 accumulation (nn.Linear / 1x1 Conv2d / MHA in_proj,
 * out_proj; vat_blocks.py:28-34, vat_lidar.py:88,93-97,117-120, vat_vision.py:118-137,
 * build_linear.py:18-19), batched over `batch` problems with element strides a_bs / w_bs / c_bs:
 *   C[z][m, n] = epi( sum_k A[z][m,k] * W[z][n,k] )     A rows lda apart, W rows ldw apart, C rows ldc apart
 *   epi(x): x += bias[n]; GELU(x) (exact erf) if flags & LVQ_GEMM_GELU, or x / (1 + exp(-1.702 x)) in fp32 if flags &
 *           LVQ_GEMM_QUICK_GELU (quick_gelu, clip_sdpa.py:73-74,182; -0 or a tiny negative value for large negative x, never NaN;
 *           both flags together: LVQ_EINVAL); x *= alpha;
 *           x += residual[z][m,n] (fp32, same layout as C) ; x += rowtab[(m % rowtab_rows), n] (fp32 [rows,N]:
 *           input-independent positional tables, geo_pe + view_embed[sid] of vat_lidar.py:235-248)
 *   outputs: c_f32 and/or c_bf16 (+ c_lo).  a_lo / w_lo both NULL (bf16) or both non-NULL (bf16x3).
 *   Requirements: k, lda, ldw, a_bs, w_bs multiples of 8; 16-byte aligned operand bases (else LVQ_EUNSUPPORTED). */
enum { LVQ_GEMM_GELU = 1, LVQ_GEMM_QUICK_GELU = 2 };
int lvq_gemm_bf16(const lvq_bf16 *a, const lvq_bf16 *a_lo, const lvq_bf16 *w, const lvq_bf16 *w_lo,
                  const float *bias, const float *residual, const float *rowtab, int64_t rowtab_rows,
                  float alpha, int flags, int64_t m, int n, int k, int64_t lda, int64_t ldw, int64_t ldc,
                  int batch, int64_t a_bs, int64_t w_bs, int64_t c_bs, float *c_f32, lvq_bf16 *c_bf16,
                  lvq_bf16 *c_lo, lvq_stream_t stream);

/* Row-complete Linear + LayerNorm (+ positional table) for the VATLiDAR token path (vat_lidar.py:222-248):
 *   Y = LayerNorm(A W^T + bias) * gamma + beta + post_add[row % post_rows, :]   -> bf16 (+ lo)
 * without materialising the fp32 [M,N] product.  Supported: n in {256,512,768,896,1024}, k % 32 == 0, k <= 256
 * (else LVQ_EUNSUPPORTED: callers use lvq_gemm_bf16 + lvq_layernorm). */
int lvq_gemm_ln_bf16(const lvq_bf16 *a, const lvq_bf16 *a_lo, const lvq_bf16 *w, const lvq_bf16 *w_lo, const float *bias,
                     const float *gamma, const float *beta, float eps, const float *post_add, int64_t post_rows,
                     int64_t m, int n, int k, int64_t lda, int64_t ldw, lvq_bf16 *y_bf16, lvq_bf16 *y_lo, lvq_stream_t stream);

/* fp32 -> bf16 (round-to-nearest-even) with optional lo part (x - bf16(x)) for the bf16x3 mode. */
int lvq_cast_bf16(const float *x, int64_t n, lvq_bf16 *hi, lvq_bf16 *lo, lvq_stream_t stream);
/* out = (hi + lo) * alpha as fp32 (lo may be NULL): hands attention outputs back to fp32 callers. */
int lvq_bf16_to_f32(const lvq_bf16 *hi, const lvq_bf16 *lo, int64_t n, float alpha, float *out, lvq_stream_t stream);

/* Attention core = F.scaled_dot_product_attention inside nn.MultiheadAttention (vat_blocks.py:39,42)
 * and deepencoder sdp_attention (clip_sdpa.py:50-66, sam_vary_sdpa.py:27-42):
 *   O[b,i,h,:] = softmax_j( Q[b,i,h,:].K[b,j,h,:] * scale + bias[b,h,i,j] ) V[b,j,h,:]
 *   element (b,i,h,e) of q lives at q[b*q_bstride + i*ldq + h*q_hstride + e] (same for k, v, o), so packed
 *   [B,N,3d] in_proj outputs and [B,H,S,D] tensors are both addressable without a copy.
 *   bias (optional, fp32 [B,H,Nq,Nkv]); causal != 0 adds the lower-triangular mask aligned to the END
 *   (query i sees keys j <= i + Nkv - Nq), used by the stand-in decoder head.  With Nq > Nkv the first Nq - Nkv queries see no
 *   key at all: their output rows (o and o_lo) are ZERO on every path (fused kernels, KV-split combine, split path).
 *   n_kv_heads < n_heads => grouped-query attention (head h reads kv head h / (n_heads/n_kv_heads)).
 *   Online softmax, statistics and accumulation in fp32.  dh multiple of 16 and <= 128: fused flash
 *   kernel, no workspace.  Larger dh (448, 1024: the reference's 2-head defaults) or dh % 16 == 8: split
 *   path (scores GEMM -> row softmax -> PV GEMM) using the workspace; needs n_heads == n_kv_heads. */
size_t lvq_attention_workspace_bytes(int batch, int n_heads, int nq, int nkv, int dh, int precision);
/* =====================================================================================
 * f1/f3  sparse BEV key stream of VATLiDAR (vat_lidar.py:212-248 + vat_blocks.py:42; csrc/bev_tiles.hip).
 * A BEV cell with an empty 3x3 neighbourhood gives a token -- and K|V rows -- that depend on the weights only.  The stream runs
 * tile-major over 8 x 8-cell tiles (64 keys each; key order is free under softmax): CLEAN tiles (no pillar in the 10 x 10 halo)
 * are read from a per-model K|V table that the caller builds once per weights version by running these same entry points on an
 * empty scene with force_all = 1 (bit-identical rows by construction), LIVE tiles are computed per scene.
 * ===================================================================================== */
/* PointPillarScatter (pointpillar_scatter.py:14-37) as an index map instead of a canvas: idx_map[b, y, x] = pillar row or -1.
 * Rows >= *n_voxels_dev (if given) are ignored. */
int lvq_pillar_index_map(const int32_t *coords_bzyx, int64_t m_cap, const int32_t *n_voxels_dev, int batch, int ny, int nx,
                         int32_t *idx_map, lvq_stream_t stream);
/* Piece / row bookkeeping.  ny, nx multiples of 8; nt = (ny/8)(nx/8) tiles of 8 x 8 cells per scene, each made of eight 2 x 4-cell
 * PIECES (piece p: row pair p >> 1, column half p & 1).  Keys run TILE-MAJOR: cell (y, x) is key 64 t + 8 p + 4 (y & 1) + (x & 3).
 * A cell is DIRTY when its 3 x 3 neighbourhood holds a pillar (its token depends on the scene); a piece is live when it has a dirty
 * cell.  The token kernel works on live pieces and stores the dirty cells' rows compactly, in (tile, scene, piece, cell) order.
 *   live_list   [batch * nt * 8]      code (t * batch + s) * 8 + p of the k-th live piece
 *   piece_dirty [batch * nt * 8][2]   per live piece k: (number of its first dirty row, its 8-bit dirty mask)
 *   row_src     [batch * ny * nx]     per (scene s, key e) at s * ny * nx + e: row_base + (dirty-row number) for a dirty cell, e (its row
 *                                     in the per-model table, which occupies rows 0 .. ny*nx-1 of the same K|V buffer) otherwise
 *   counts      [3]                   live pieces, rows of the live pieces (8 x), dirty rows
 * force_all != 0 marks every cell dirty (table build with row_base = 0; dense comparator).
 * Reference: the key / value tokens of vat_lidar.py:222-248, which this bookkeeping lets the kernels compute for the dirty cells only. */
size_t lvq_bev_tiles_workspace_bytes(int batch, int ny, int nx);
int lvq_bev_tiles(const int32_t *idx_map, int batch, int ny, int nx, int force_all, int row_base, int32_t *live_list, int32_t *piece_dirty,
                  int32_t *row_src, int32_t *counts, void *ws, size_t ws_bytes, lvq_stream_t stream);
/* Tokens of the dirty cells, fused: pillar gather + depthwise 3x3 + GELU (refine, vat_lidar.py:212-221; tap order and fmaf chain of
 * lvq_dwconv3x3_gelu) -> 1x1 conv (proj) -> LayerNorm (norm_tokens) -> + positional table (pe_tiled [ny*nx, n] fp32 in tile-major
 * row order).  x [dirty rows, n]: the compact rows numbered by lvq_bev_tiles (capacity cap_tiles * 64).  w_lo != NULL: conv
 * tokens and W as hi + lo (three products); x_lo != NULL additionally stores the lo half of x.  c_in = 64, n in {256, 512, 768,
 * 1024} (else LVQ_EUNSUPPORTED: use lvq_pillar_dwconv3x3_gelu + lvq_gemm_ln_bf16). */
int lvq_bev_tile_tokens(const float *pillar_feat, const int32_t *idx_map, const int32_t *live_list, const int32_t *piece_dirty,
                        const int32_t *counts, int64_t cap_tiles, int batch, int ny, int nx, int c_in, const float *w9, const float *b9, const lvq_bf16 *w,
                        const lvq_bf16 *w_lo, const float *bias, const float *gamma, const float *beta, float eps, const float *pe_tiled,
                        int n, lvq_bf16 *x, lvq_bf16 *x_lo, lvq_stream_t stream);
/* K|V rows of the dirty cells straight from the pillar features, without the d-wide token (csrc/bev_tiles.hip: k_tile_kv).  LayerNorm of
 * a linear map of the 64-channel conv token t = GELU(dwconv3x3(pillars)) is a per-row rescale of another linear map of t, so
 *     K|V = W_kv (LayerNorm(Wp t + bp) + PE[key]) + b_kv = rstd (M t + m0) + T[key],   rstd = 1 / sqrt((|R t + r0|^2 + c0) / d_ln + eps)
 * with M = W_kv diag(gamma) Wc [2 n, 64], m0 = W_kv (gamma * bc) [2 n], T[key] = W_kv (beta + PE[key]) + b_kv [ny*nx (tile-major), 2 n] fp32,
 * (Wc, bc) = (Wp, bp) minus their means over the d_ln outputs, R [64, 64] the triangular factor of [Wc bc] (c0 = its corner squared):
 * vat_lidar.py:222-248 + vat_blocks.py:42 folded once per weights version (exact algebra; the 768-deep projection becomes 64-deep).
 * m_lo / r_lo != NULL: t, M and R as hi + lo (three products).  kv [dirty rows, 2 n] bf16: the compact rows numbered by lvq_bev_tiles.
 * ws != NULL (lvq_bev_tile_kv_workspace_bytes(cap_tiles)): two launches -- k_conv_rows stores (t, rstd, key) of the dirty rows, k_kv_rows
 * projects contiguous 64-row tiles -- instead of the single kernel; the same arithmetic, bit-identical rows.  k_fp16 != 0 (two-launch
 * form only): the K half (columns 0 .. n-1) is stored as IEEE fp16 for the fp16 Q K^T pass of the attention entry points.
 * t_f16 != 0 (two-launch form only): t_tiled holds IEEE fp16 instead of fp32 (half the bytes of the kernel's largest read stream; the
 * caller guarantees |T| < 65504 -- its rounding, 2^-12, disappears under the bf16 rounding of the rows). */
size_t lvq_bev_tile_kv_workspace_bytes(int64_t cap_tiles);
int lvq_bev_tile_kv(const float *pillar_feat, const int32_t *idx_map, const int32_t *live_list, const int32_t *piece_dirty,
                    const int32_t *counts, int64_t cap_tiles, int batch, int ny, int nx, int c_in, const float *w9, const float *b9,
                    const lvq_bf16 *m, const lvq_bf16 *m_lo, const float *m0, const lvq_bf16 *r, const lvq_bf16 *r_lo, const float *r0, float c0,
                    int d_ln, float eps, const void *t_tiled, int t_f16, int n, int k_fp16, lvq_bf16 *kv, void *ws, size_t ws_bytes,
                    lvq_stream_t stream);
/* c[0 .. *m_rows_dev) = a @ w^T + bias over the live rows only (the row count stays on the device; vat_blocks.py:42: the K|V
 * projection inside `ca`, restricted to the rows that differ from the per-model table); m_cap, n multiples of 256, k of 64.  Operand forms as lvq_gemm_bf16 (plain | a plain, w hi + lo | both hi + lo). */
int lvq_gemm_bf16_live_rows(const lvq_bf16 *a, const lvq_bf16 *a_lo, const lvq_bf16 *w, const lvq_bf16 *w_lo, const float *bias,
                            int64_t m_cap, const int32_t *m_rows_dev, int n, int k, int64_t lda, int64_t ldw, int64_t ldc,
                            lvq_bf16 *c_bf16, lvq_bf16 *c_lo, lvq_stream_t stream);
/* vat_blocks.py:41-42 for VATLiDAR's key stream (vat_lidar.py:272-285): softmax(q K^T * scale) V over the tiled stream: key slot r (0..63) of tile t of batch b is row row_src[(b * n_tiles + t) * 64 + r] of
 * k_rows / v_rows -- ONE K|V buffer holding the per-model table rows and the computed rows of every batch (lvq_bev_tiles' row_src).
 * Shapes of lvq_attention_stream_ok(nq, 64 * n_tiles, 64) only; q plain or hi + lo (mixed mode), K / V plain.
 * k_fp16 != 0 ("mixed16"): the K columns of the buffer hold IEEE fp16 (lvq_bev_tile_kv with k_fp16), q (hi + lo summed) is rounded once
 * to fp16 and Q K^T runs as ONE fp16 MFMA pass; P and V stay bf16.  The caller guarantees |K|, |q * scale * log2 e| < 65504.
 * Workspace: lvq_attention_workspace_bytes(batch, n_heads, nq, 64 * n_tiles, 64, 1). */
int lvq_attention_bf16_tiled(const lvq_bf16 *q, const lvq_bf16 *q_lo, const lvq_bf16 *k_rows, const lvq_bf16 *v_rows, const int32_t *row_src,
                             int batch, int n_heads, int nq, int n_tiles, int dh, int64_t q_bstride, int64_t ldq, int64_t q_hstride,
                             int64_t ldkv, int64_t kv_hstride, int64_t o_bstride, int64_t ldo, int64_t o_hstride, float scale, int k_fp16,
                             lvq_bf16 *o, lvq_bf16 *o_lo, void *ws, size_t ws_bytes, lvq_stream_t stream);

/* Attention over the DIRTY rows only, for queries that do not depend on the batch (VATLiDAR's first block, vat_lidar.py:259-270 (q = self.query expanded over the batch + view embedding) and 283-288 (blocks) +
 * vat_blocks.py:37-42: learned queries -> self-attention -> ca_ln -> W_q).  With the fixed softmax reference the contribution of a
 * table key to (l, O) is then the same for every batch, so  result = TOTALS(all table keys) - table terms at the batch's dirty
 * cells + its computed rows: a stream over 2 x (dirty fraction) of the keys.
 *   lvq_attention_bf16_stream_totals: totals [n_heads, nq, dh + 2] fp32 = unnormalised (O | m | l) of ONE batch of queries over a
 *       dense key stream (the per-model K | V table); once per weights version.
 *   lvq_bev_scene_pairs: pair_src [batch, cap_tiles, 64], pair_info [batch, 2] from lvq_bev_tiles' row_src -- tile j of a batch holds
 *       its dirty rows 32 j .. 32 j + 31 (keys 0..31, added) and the table rows of the same cells (keys 32..63, subtracted);
 *       pair_info[2 b] = pair tiles, pair_info[2 b + 1] = 1 when that is shorter than the full stream (else the batch runs row_src).
 *       Contents of pair_src beyond a batch's list are unspecified (with cap_tiles >= n_tiles the last tile slot of every batch is
 *       scratch of the call: a list that is used has fewer than n_tiles tiles).
 *   lvq_attention_bf16_tiled_signed: as lvq_attention_bf16_tiled (same q as the totals; q_bstride = 0 shares one copy).  A
 *       (batch, head) whose signed row sum is not finite or below 1/16 of the table total is redone over its full stream by a
 *       predicated second launch.  Not bit-identical to the full stream (fp32 accumulation order); same operand roundings -- EXCEPT with
 *       k_fp16 ("mixed16"): the totals may have been taken with the full query (k_fp16 = 2: fp16 hi + lo, the default of the Python mirror)
 *       while the per-scene streams subtract the table rows with the once-rounded fp16 query, so the subtraction cancels only up to that
 *       rounding (2^-11 of each subtracted score; grows with the dirty fraction, < 50 % by construction).  Deliberate: the clean 70 % of
 *       the keys then never see the rounded query (5.6e-4 -> 2.8e-4 on the bench scene); pass k_fp16 = 1 to the totals for exact
 *       cancellation.  The 1/16 trigger above was derived for fp32 ordering error only and is not a bound for this mode: mixed16 is
 *       held to the 1e-3 bar by tests (tests/test_gpu_tiled_stream.py, tests/test_gpu_pipeline.py), not by that trigger. */
size_t lvq_attention_stream_totals_workspace_bytes(int n_heads, int nq, int nkv, int dh);
int lvq_attention_bf16_stream_totals(const lvq_bf16 *q, const lvq_bf16 *q_lo, const lvq_bf16 *k, const lvq_bf16 *v, int n_heads, int nq,
                                     int nkv, int dh, int64_t ldq, int64_t q_hstride, int64_t ldkv, int64_t kv_hstride, float scale, int k_fp16,
                                     float *totals, void *ws, size_t ws_bytes, lvq_stream_t stream);
int lvq_bev_scene_pairs(const int32_t *row_src, int batch, int n_tiles, int row_base, int cap_tiles, int32_t *pair_src, int32_t *pair_info,
                        lvq_stream_t stream);
size_t lvq_attention_tiled_signed_workspace_bytes(int batch, int n_heads, int nq, int n_tiles, int dh);
int lvq_attention_bf16_tiled_signed(const lvq_bf16 *q, const lvq_bf16 *q_lo, const lvq_bf16 *k_rows, const lvq_bf16 *v_rows,
                                    const int32_t *row_src, const int32_t *pair_src, const int32_t *pair_info, int pair_cap_tiles, const float *totals, int batch, int n_heads, int nq,
                                    int n_tiles, int dh, int64_t q_bstride, int64_t ldq, int64_t q_hstride, int64_t ldkv,
                                    int64_t kv_hstride, int64_t o_bstride, int64_t ldo, int64_t o_hstride, float scale, int k_fp16, lvq_bf16 *o,
                                    lvq_bf16 *o_lo, int32_t *stats, void *ws, size_t ws_bytes, lvq_stream_t stream);

/* Shared subtraction: the signed stream for a batch whose scenes have dirty cells in common (one sensor rig: ego surroundings, near-field
 * ground).  A cell dirty in m of the batch's S scenes with 2 m > S + 1 is in the shared set G: its table row is subtracted ONCE per call (a
 * B = 1 stream over the G list gives BASE = TOTALS - sum over G) and added back, as a plain key, in the S - m scenes where it is clean.
 * Nothing is kept between calls; a batch without common cells gets an empty G and the lists and results of the two functions above.
 * Cost rule, taken on the device from the counts: with a(s) / b(s) the tiles scene s streams with its plain pair list / with the shared lists
 * (n_tiles when a list is not shorter than the full stream), G is used only when sum_s (a(s) - b(s)) exceeds the tiles of the G list;
 * otherwise G counts as empty (a batch of mostly dirty scenes has a large G that hardly shortens any list).
 *   lvq_bev_shared_lists: list_src [batch + 1, cap_tiles, 64] (cap_tiles >= n_tiles), list_info [batch + 1, 4]; entry `batch` is the G list.
 *       A scene's list, in order: pair tiles (keys 0..31 = computed rows of its dirty cells outside G, keys 32..63 = the table rows of the
 *       same cells, subtracted; last one padded with row 0 in both halves) | tiles of 64 plus keys, one per cell of G in key order (the
 *       computed row where the scene is dirty, the table row where it is clean) | at most two remainder tiles of 32 plus keys whose keys
 *       32..63 are ignored (row 0).  Every list has |G| plus keys, padded to a multiple of 32 with table row 0 -- the G list too, so the
 *       padding is subtracted once and added back by every scene.  list_info[4 b] = tiles, [4 b + 1] = 1 when the list is shorter than the
 *       full stream (else the batch runs row_src and ignores BASE), [4 b + 2] = first tile whose keys 32..63 are added (= pair tiles),
 *       [4 b + 3] = first tile whose keys 32..63 are ignored.  Workspace: 64 n_tiles + 512 (batch + 1) + 512 bytes.
 *   lvq_attention_bf16_tiled_shared: as lvq_attention_bf16_tiled_signed with those lists (one copy of q for all batches);
 *       totals_k_fp16 = the k_fp16 the totals were taken with (the G stream uses the same operand form).  The cancellation check and
 *       the guard statistics judge against TOTALS as before.  Workspace: lvq_attention_tiled_signed_workspace_bytes (covers both). */
int lvq_bev_shared_lists(const int32_t *row_src, int batch, int n_tiles, int row_base, int cap_tiles, int32_t *list_src, int32_t *list_info,
                         void *ws, size_t ws_bytes, lvq_stream_t stream);
int lvq_attention_bf16_tiled_shared(const lvq_bf16 *q, const lvq_bf16 *q_lo, const lvq_bf16 *k_rows, const lvq_bf16 *v_rows,
                                    const int32_t *row_src, const int32_t *list_src, const int32_t *list_info, int list_cap_tiles,
                                    const float *totals, int totals_k_fp16, int batch, int n_heads, int nq, int n_tiles, int dh,
                                    int64_t ldq, int64_t q_hstride, int64_t ldkv, int64_t kv_hstride, int64_t o_bstride, int64_t ldo,
                                    int64_t o_hstride, float scale, int k_fp16, lvq_bf16 *o, lvq_bf16 *o_lo, int32_t *stats, void *ws,
                                    size_t ws_bytes, lvq_stream_t stream);

/* Guard of the plain-bf16 key stream ("mixed" modes), per-model half: g[h * nq + i] = (1 + max_k |scale q_i . k_k|) / sqrt(N_eff)
 * with N_eff = (sum_k p_k)^2 / sum_k p_k^2, p = softmax weights of query i of head h over the nkv key rows (head_dim 64, nkv % 4 == 0; plain
 * bf16 operands -- a statistic, not a result).  The error that plain K / V / P leave in the attention output grows like max(g)
 * (tools/mixed_guard_study.py); the caller keeps the plain stream only while max(g) stays under its threshold and otherwise runs hi + lo
 * operands.  The per-launch half is lvq_attention_bf16_tiled_signed's `stats` (NULL or four int32 words that are accumulated into: [0] count of
 * (scene, head, query) rows whose row sum exceeds 1.5x the table's -- the softmax mass moved onto the scene's own keys, which the per-model
 * statistic has not seen; [1] (batch, head) pairs re-run by the cancellation check; [2] the largest row sum / table row sum seen, as float
 * bits; [3] unused). */
size_t lvq_stream_guard_workspace_bytes(int nq, int64_t nkv);
int lvq_stream_guard(const lvq_bf16 *q, const lvq_bf16 *k_rows, int n_heads, int nq, int64_t nkv, int64_t ldq, int64_t ldk, float scale, float *g,
                     void *ws, size_t ws_bytes, lvq_stream_t stream);

/* nn.MultiheadAttention's scaled-dot-product core (vat_blocks.py:39,42; clip_sdpa.py:50-66; sam_vary_sdpa.py:27-42) and its shape query:
 * 1 when the long-stream kernel takes (nq, nkv, dh) without bias / mask: head_dim 64, nkv >= 4096 and a multiple of 64, query
 * count with at most 1/8 padding to 128 / 192 rows.  Those are the shapes for which lvq_attention_bf16 accepts the "mixed" operand
 * form q = hi + lo, k / v plain (k_lo = v_lo = NULL): Q-side rounding is common to all keys of a row and does not average out
 * over the stream, K / V / P roundings do.  Any other shape with that operand form returns LVQ_EUNSUPPORTED. */
int lvq_attention_stream_ok(int nq, int nkv, int dh);
int lvq_attention_bf16(const lvq_bf16 *q, const lvq_bf16 *q_lo, const lvq_bf16 *k, const lvq_bf16 *k_lo,
                       const lvq_bf16 *v, const lvq_bf16 *v_lo, const float *bias, int batch, int n_heads,
                       int n_kv_heads, int nq, int nkv, int dh, int64_t q_bstride, int64_t ldq, int64_t q_hstride,
                       int64_t k_bstride, int64_t ldk, int64_t k_hstride, int64_t v_bstride, int64_t ldv,
                       int64_t v_hstride, int64_t o_bstride, int64_t ldo, int64_t o_hstride, float scale, int causal,
                       lvq_bf16 *o, lvq_bf16 *o_lo, void *ws, size_t ws_bytes, lvq_stream_t stream);

/* ---- Grid self-attention with the decomposed relative-position bias (csrc/vit_attention.hip) ---------------------------------
 * The attention of the SAM / ViTDet image encoder (deepencoder/sam_vary_sdpa.py:269-296 with add_decomposed_rel_pos 382-413 and
 * get_rel_pos 348-379 at q_size == k_size), for a windowed block (grid = one window) and a global block (grid = the image) alike:
 *   O[b, i, h, :] = softmax_j( scale q_i.k_j + q_i.Rh[y_i - y_j + gh - 1] + q_i.Rw[x_i - x_j + gw - 1] ) v_j
 *   i = y_i gw + x_i, j = y_j gw + x_j over the gh x gw grid of batch entry b; the bias terms use the UNSCALED q; statistics and
 *   accumulation in fp32.  The bias is formed inside the kernel from the two tables: no array of size (gh gw)^2 is read or written.
 *   qkv     the packed projection as Attention.qkv emits it: [batch * gh * gw, 3 * n_heads * dh] rows ld_qkv apart (elements),
 *           column = part * n_heads * dh + h * dh + e, part 0 / 1 / 2 = q / k / v
 *   rel_h   [2 gh - 1, dh], rel_w [2 gw - 1, dh], dense rows (tables of another length are resized by the caller, once per weights)
 *   o       [batch * gh * gw, n_heads * dh] rows ldo apart: the A operand of the output projection; o_lo (optional) = fp32 result - o
 *   forms   qkv_lo, rel_h_lo, rel_w_lo all NULL: plain bf16; all non-NULL: bf16x3 (scores, bias products and P V as hi + lo)
 * Family: dh == 64, 1 <= gh, gw <= 64, any batch and head count; otherwise LVQ_EUNSUPPORTED (lvq_attention_relpos_ok is that rule).
 * ld_qkv a multiple of 8, ldo of 4, 16-byte aligned operands, 8-byte aligned outputs (else LVQ_EUNSUPPORTED); ws_bytes below
 * lvq_attention_relpos_workspace_bytes: LVQ_EWORKSPACE.  Every refusal happens before any launch, outputs untouched.
 * lvq_attention_relpos_plan (host only, a hook for tests): what a call on a gh x gw grid launches -- *stages = K | V stages in LDS (1 or 2),
 * *lds_bytes = its dynamic LDS request; precision 1 (plain) or 3 (hi + lo), else LVQ_EINVAL; a grid outside the family LVQ_EUNSUPPORTED. */
int lvq_attention_relpos_ok(int gh, int gw, int dh);
int lvq_attention_relpos_plan(int gh, int gw, int precision, int *stages, size_t *lds_bytes);
size_t lvq_attention_relpos_workspace_bytes(int batch, int n_heads, int gh, int gw, int dh, int precision);
int lvq_attention_relpos_bf16(const lvq_bf16 *qkv, const lvq_bf16 *qkv_lo, int64_t ld_qkv, const lvq_bf16 *rel_h,
                              const lvq_bf16 *rel_h_lo, const lvq_bf16 *rel_w, const lvq_bf16 *rel_w_lo, int batch, int n_heads,
                              int gh, int gw, int dh, float scale, lvq_bf16 *o, lvq_bf16 *o_lo, int64_t ldo, void *ws,
                              size_t ws_bytes, lvq_stream_t stream);

/* ---- Embedding step of the CLIP-L tower on channel-major patch features (csrc/clip_embed.hip) -----------------------------------
 * CLIPVisionEmbeddings.forward + VitModel.pre_layrnorm (deepencoder/clip_sdpa.py:147-169, 362-363) in one transposing launch, and
 * with it the token-major copy of the same features that the projector reads (deepencoder_infer.py: sam_feats.flatten(2).permute):
 *   feat    [batch, c, hw] fp32   channel-major patch features (SAM's output, or the tower's own patch conv's)
 *   cls     [c] fp32              class_embedding
 *   pos     [1 + hw, c] fp32      position table ALREADY at this grid (get_abs_pos is input-independent: the caller resamples it)
 *   gamma, beta [c] (beta may be NULL), eps      pre_layrnorm
 *   hidden  [batch * (1 + hw), c] fp32 = LayerNorm(cat(cls, feat^T) + pos): row b (1 + hw) is the class row of image b
 *   tok_hi, tok_lo (optional)  [batch * hw, ld_tok] bf16 = feat^T as a GEMM operand, exactly lvq_cast_bf16 of the transposed array
 *           (hi, and lo = x - hi when tok_lo is given); columns c .. ld_tok - 1 are not written
 * Statistics are fp32 and centred (mean first, then the sum of squared differences), as in lvq_layernorm.
 * Family: c % 64 == 0, c <= 2048, hw >= 1, batch >= 1 (lvq_clip_embed_ok is that rule); otherwise LVQ_EUNSUPPORTED.  16-byte aligned
 * feat / cls / pos / gamma / beta / hidden, 4-byte aligned tok_hi / tok_lo, ld_tok even and >= c, batch * (1 + hw) < 2^31 (else
 * LVQ_EUNSUPPORTED); tok_lo without tok_hi: LVQ_EINVAL.  No workspace.  Every refusal happens before any launch, outputs untouched. */
int lvq_clip_embed_ok(int batch, int c, int hw);
int lvq_clip_embed(const float *feat, const float *cls, const float *pos, const float *gamma, const float *beta, float eps,
                   int batch, int c, int hw, float *hidden, lvq_bf16 *tok_hi, lvq_bf16 *tok_lo, int64_t ld_tok,
                   lvq_stream_t stream);

/* ---- Fused short-K/V cross-attention sub-path (csrc/cross_fused.hip) -------------------------------------------------------
 * out = q + ca(ca_ln(q), kv, kv): encoder-decoder/training/models/vat_blocks.py:41-42 (nn.LayerNorm + nn.MultiheadAttention with
 * batch_first, eval mode) as TWO launches: the K|V projection of the kv tokens (written straight in MFMA fragment order into `ws`)
 * and one kernel that takes the fp32 queries through LayerNorm, the Q projection, softmax(Q K^T / sqrt(dh)) V, the out projection,
 * bias and the fp32 residual without an activation round trip through HBM.  BASELINE.json's metric shape is
 * (batch, nq, nkv, d, n_heads) = (1, 32768, 196, 768, 12).
 *   lvq_ca_fused_ok       1 for the shapes the kernel family takes: d = 768, n_heads = 12 (head_dim 64), nq % 32 == 0, 192 < nkv <= 224 (seven 32-key blocks: the only instantiation).
 *   lvq_ca_fused_pack     once per weights version: ln_gamma / ln_beta [d] (ca_ln), in_proj_w [3d, d], in_proj_b [3d], out_w [d, d],
 *                         out_b [d] (ca.in_proj_weight / in_proj_bias / out_proj.*) -> `packed` (lvq_ca_fused_packed_bytes): MFMA-fragment-
 *                         major 16-bit copies (gamma folded into W_q, beta and 1/sqrt(dh) into its bias).  f16 = 0: bf16 operands;
 *                         f16 = 1: IEEE fp16 operands (same MFMA rate, 8x smaller operand rounding: the form that meets the 1e-3 parity
 *                         bar, tools/precision_study_ca.py; values that are not bounded by construction are clamped to +-65504).
 *                         A blob packed with one f16 value must be used with the same value.
 *   lvq_ca_fused          q [batch, nq, d] fp32, kv [batch, nkv, d] fp32 -> out [batch, nq, d] fp32 (out may not alias q).
 * All pointers are device pointers; stream-ordered; `ws` (lvq_ca_fused_workspace_bytes) is scratch for the packed K | V^T. */
int lvq_ca_fused_ok(int batch, int nq, int nkv, int d, int n_heads);
size_t lvq_ca_fused_packed_bytes(int d, int n_heads);
size_t lvq_ca_fused_workspace_bytes(int batch, int nq, int nkv, int d, int n_heads);
int lvq_ca_fused_pack(const float *ln_gamma, const float *ln_beta, const float *in_proj_w, const float *in_proj_b, const float *out_w,
                      const float *out_b, int d, int n_heads, int f16, void *packed, size_t packed_bytes, lvq_stream_t stream);
int lvq_ca_fused(const float *q, const float *kv, const void *packed, float eps, int batch, int nq, int nkv, int d, int n_heads, int f16,
                 float *out, void *ws, size_t ws_bytes, lvq_stream_t stream);

/* The inverse of lvq_pillar_scatter: the occupied cells of a dense BEV canvas [batch, c, h, w] (fp32) as pillars -- feats [cap, c], coords (b, 0, y, x)
 * [cap, 4], *n_cells = their number (zeroed by the call; may exceed cap: rows past cap are not written).  A cell whose c channels are all zero is exactly an
 * absent pillar for VATLiDAR's refine conv, so VATLiDAR.forward(bev) -- the reference's own entry point (vat_lidar.py:187-304; the fp16 .npy canvases of
 * precompute_bev_features.py:391-395 are mostly empty) -- can take the sparse key stream of lvq_bev_tile_kv.  Row order follows the allocation atomics
 * (not reproducible); everything downstream addresses pillars through coordinates.  The reference has no counterpart: it always runs the dense canvas. */
int lvq_bev_occupied_cells(const float *bev, int batch, int c, int h, int w, int64_t cap, float *feats, int32_t *coords_bzyx, int32_t *n_cells,
                           lvq_stream_t stream);

/* VATLiDAR front (vat_lidar.py:82-85,212): depthwise Conv2d(C,C,3,pad=1,groups=C) + exact GELU on
 * NCHW fp32 input, written TOKEN-MAJOR [B, H*W, C] as bf16 (the A operand of the 1x1-conv GEMM). */
int lvq_dwconv3x3_gelu(const float *bev, const float *w9, const float *bias, int batch, int ch, int h, int w,
                       lvq_bf16 *tokens_hi, lvq_bf16 *tokens_lo, lvq_stream_t stream);

/* Sparse BEV bridge = PointPillarScatter.forward (pointpillar_scatter.py:14-37) followed by VATLiDAR.refine
 * (vat_lidar.py:212-221: depthwise 3x3 conv, padding 1, + GELU) and the flatten to tokens [batch*ny*nx, ch], WITHOUT
 * materialising the dense [batch, ch, ny, nx] canvas: only an int32 index map (pillar row or -1) is scattered into `ws`.
 * Bit-identical to lvq_pillar_scatter + lvq_dwconv3x3_gelu.  feat [m_cap, ch] fp32, coords (b, z, y, x) with nz == 1,
 * rows >= *n_voxels_dev skipped (NULL = all m_cap rows).  tokens_lo may be NULL (plain bf16). */
size_t lvq_pillar_dwconv_workspace_bytes(int batch, int ny, int nx);
int lvq_pillar_dwconv3x3_gelu(const float *feat, const int32_t *coords_bzyx, int64_t m_cap, const int32_t *n_voxels_dev,
                              int ch, int batch, int ny, int nx, const float *w9, const float *bias, lvq_bf16 *tokens_hi,
                              lvq_bf16 *tokens_lo, void *ws, size_t ws_bytes, lvq_stream_t stream);

/* out[r, :] = x[r, :] * alpha + add[(r % add_rows), :]  (query = query + view_embed chunk,
 * vat_lidar.py:259-270; prefix * prefix_scale, trainer.py:581,594) -- fp32 elementwise; add may be NULL. */
int lvq_scale_add_rows(const float *x, const float *add, int64_t add_rows, float alpha, int64_t rows, int d,
                       float *out, lvq_stream_t stream);

/* Stand-in decoder head pieces (Qwen2-style; validation.py:146-156 drives `base(inputs_embeds, labels)`):
 * RMSNorm, rotary embedding applied in place to a packed projection (rows = B*L, position = row % seq_len),
 * SiLU(gate)*up on a packed [rows, 2*inter] gate|up projection, and the shifted-label cross entropy. */
int lvq_rmsnorm(const float *x, const float *gamma, float eps, int64_t rows, int d, float *y_f32, lvq_bf16 *y_bf16,
                lvq_bf16 *y_lo, lvq_stream_t stream);
int lvq_rope_inplace(lvq_bf16 *x, lvq_bf16 *x_lo, int64_t rows, int seq_len, int n_heads, int dh, int64_t ld, float theta,
                     lvq_stream_t stream);
/* decode-time rotary embedding (inference_engine.py:283-296 -> HF generate with a KV cache): the rows are the
 * new positions pos0 .. pos0 + seq_len - 1 of every sequence (position = pos0 + row % seq_len). */
int lvq_rope_inplace_at(lvq_bf16 *x, lvq_bf16 *x_lo, int64_t rows, int seq_len, int pos0, int n_heads, int dh, int64_t ld,
                        float theta, lvq_stream_t stream);
/* greedy decoding (inference_engine.py:283-296 with do_sample = False): out_idx[r] = index of the first maximum of x[r, 0..n)
 * (torch.argmax on finite logits). */
int lvq_argmax_rows(const float *x, int64_t rows, int n, int64_t *out_idx, lvq_stream_t stream);
/* e   payload of the per-step all-reduce (training/utils/distributed.py:7-26, commu_utils.py:148-168): out[c] = sum over rows of
 * x[r, c], fp32, in a fixed (run-to-run identical) order.  rows = 0 gives zeros. */
size_t lvq_colsum_workspace_bytes(int64_t rows, int d);
int lvq_colsum(const float *x, int64_t rows, int d, float *out, void *ws, size_t ws_bytes, lvq_stream_t stream);
/* f4  one sampling step of `base_model.generate(do_sample=True, temperature=, top_k=, top_p=)` (the reference's default call,
 * inference_engine.py:236-240,283-296 -> transformers' TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, softmax,
 * multinomial): out_idx[r] ~ softmax(logits[r] / temperature) restricted to the top_k largest logits (ties kept) and then to
 * the smallest set of largest probabilities whose mass reaches top_p; the draw is the inverse CDF at u[r] in [0, 1) (the
 * caller's RNG stream).  temperature > 0, 0 < top_p <= 1; top_k <= 0 or > vocab disables the top-k filter, which is only
 * supported for vocab <= 1024 (effective top_k <= 1024, else LVQ_EUNSUPPORTED). */
int lvq_sample_rows(const float *logits, int64_t rows, int vocab, float temperature, int top_k, float top_p, const float *u,
                    int64_t *out_idx, lvq_stream_t stream);
int lvq_swiglu(const float *gate_up, int64_t rows, int inter, lvq_bf16 *out_hi, lvq_bf16 *out_lo, lvq_stream_t stream);
/* (trainer.py:674-675 / validation.py:105-158: `out.loss` of base(inputs_embeds, labels))
 * sum over rows with labels[row] >= 0 of (logsumexp(logits[row]) - logits[row, label]) and their count:
 * loss = loss_sum_cnt[0] / loss_sum_cnt[1] (transformers causal-LM loss; labels already shifted by the
 * caller, -100 = ignore).  loss_sum_cnt [2] fp32 must be zero on entry. */
int lvq_cross_entropy(const float *logits, const int64_t *labels, int64_t rows, int vocab, float *loss_sum_cnt,
                      lvq_stream_t stream);

/* =====================================================================================
 * Data formats either side of the sparse backbone
 * ===================================================================================== */

/* f2  encoder-decoder/training/data/dataset.py:139-146: `torch.from_numpy(np.load(path)).float()` of the stored fp16 BEV
 * [C,H,W] (writer: get-data/precompute_bev_features.py:391-395).  dst[i] = (float)src[i], exact.  src/dst 16-byte aligned. */
int lvq_f16_to_f32(const uint16_t *src, float *dst, int64_t n, lvq_stream_t stream);

/* f3  pcdet/models/backbones_3d/spconv_backbone_voxelnext.py:149-164  VoxelResBackBone8xVoxelNeXt.bev_out:
 *   indices_cat = indices[:, [0, 2, 3]];  indices_unique, inv = torch.unique(indices_cat, dim=0, return_inverse=True)
 *   features_unique = zeros(len(indices_unique), C).index_add_(0, inv, features)
 * indices_bzyx [m,4] int32 (b, z, y, x), feats [m,c] fp32, grid (ny, nx) = spatial_shape[1:].
 *   out_indices_byx [cap,3] int32: unique (b, y, x) rows in ascending lexicographic order (= torch.unique(dim=0))
 *   out_feats [cap,c] fp32: rows [0, counts[0]) are written; every row is the sum of its contributors in ascending input-row
 *   order (the order of the CPU index_add_: deterministic, bit-identical to it; the CUDA index_add_ of the reference is atomic)
 *   unq_inv [m] int32: row of out_* each input row was added to;  counts [2] int32: counts[0] = number of unique rows
 *   cap >= min(m, batch*ny*nx).  batch*ny*nx must stay below 2^31 (LVQ_EOVERFLOW). */
size_t lvq_sparse_bev_merge_workspace_bytes(int64_t m, int batch, int ny, int nx);
int lvq_sparse_bev_merge(const int32_t *indices_bzyx, const float *feats, int64_t m, int c, int batch, int ny, int nx,
                         int32_t *out_indices_byx, float *out_feats, int32_t *unq_inv, int32_t *counts, void *ws,
                         size_t ws_bytes, lvq_stream_t stream);

/* f3  pcdet/models/backbones_2d/map_to_bev/height_compression.py:10-26  HeightCompression.forward:
 * SparseConvTensor.dense() -> [N, C, D, H, W] -> view(N, C*D, H, W), i.e. out[b, ch*d + z, y, x] = feats[r, ch].
 * indices [m_cap, index_cols] int32: index_cols == 4 -> (b, z, y, x); index_cols == 3 -> (b, y, x) with d == 1 (the
 * `.dense()` of the 2-D tensor bev_out returns, stored by precompute_bev_features.py).  Every element of out is written
 * (zeros where no row points); rows >= *n_live_dev are skipped (NULL = all m_cap rows).  ws holds an int32 row map
 * [batch, d, h, w]. */
size_t lvq_sparse_to_dense_workspace_bytes(int batch, int d, int h, int w);
int lvq_sparse_to_dense(const float *feats, const int32_t *indices, int index_cols, int64_t m_cap, const int32_t *n_live_dev,
                        int c, int batch, int d, int h, int w, float *out, void *ws, size_t ws_bytes, lvq_stream_t stream);

/* =====================================================================================
 * Sparse convolution backbones (csrc/sparse_conv.hip): the layers of VoxelResBackBone8xVoxelNeXt, VoxelBackBone8x / VoxelResBackBone8x
 * and PillarBackBone8x / PillarRes18BackBone8x
 * ===================================================================================== */

/* Semantics (spconv 2.x, as pcdet/models/backbones_3d/spconv_backbone_voxelnext.py:8-225, spconv_backbone.py:8-295 and spconv_backbone_2d.py:8-300
 * use it through pcdet/utils/spconv_utils.py:1-30).
 *   tensor    features [N, C] fp32, indices [N, 1 + nd] int32 = (b, z, y, x) or (b, y, x), spatial_shape (D, H, W) or (H, W), batch.
 *             The index rows of one tensor are distinct (as spconv requires); a row outside the grid or the batch takes no part.
 *   weight    [C_out, kz, ky, kx, C_in] (2-D: [C_out, ky, kx, C_in]), spconv 2.x's layout.  The convolution is a CROSS-CORRELATION: it
 *             equals torch.nn.functional.conv3d(dense input, weight.permute(0, 4, 1, 2, 3)).  Kernel offset o = (oz * ky + oy) * kx + ox.
 *   submanifold conv (SubMConv3d / SubMConv2d; odd kernel <= 3, stride 1): the output rows are the input rows, in the same order;
 *             out[i] = bias + sum_o W[:, o, :] . in[row(c_i + o - k/2)] over the offsets whose neighbour is an active row of the same
 *             scene inside the grid.  An absent neighbour contributes nothing.
 *   regular conv (SparseConv3d / SparseConv2d; kernel <= 3, stride s, padding p >= 0, each per axis): output shape floor((D + 2p - k) / s) + 1 per
 *             axis; site q is active iff some input q * s - p + o is active and inside the grid; out[q] = sum_o W[:, o, :] . in[row(q * s - p + o)].
 *             spconv leaves the order of the output rows unspecified; here they ascend in (b, z, y, x).  Everything downstream
 *             (lvq_sparse_bev_merge, lvq_sparse_to_dense, further rules) addresses rows through their coordinates.
 *   epilogue  y = [relu]((acc + bias) * scale + shift [+ residual[i]]),  scale = gamma / sqrt(var + eps), shift = beta - mean * scale of
 *             an eval-mode BatchNorm1d (eps 1e-3 in the backbone, 1e-5 in shared_conv's default nn.BatchNorm1d).
 *   order     offsets are summed in ascending o for every row, channels in ascending order inside an offset, fp32 accumulation; a
 *             row's bits depend on its own neighbours only -- not on its tile or its position: permuting the input rows of a
 *             submanifold conv permutes the output rows bit for bit, and two runs give the same bits (no atomics on outputs).
 *
 * lvq_sparse_conv_rules: the active output set and the neighbour table of one layer geometry (spconv's "indice pairs"; layers that share
 * an indice_key share one table).
 *   indices        [n_in, 1 + ndim] int32;  spatial_shape / kernel / stride / padding: HOST int32[ndim] in (z, y, x) or (y, x) order
 *                  (stride / padding are ignored, and may be NULL, for subm != 0)
 *   out_indices    [out_cap, 1 + ndim] int32, ascending (b, z, y, x); not touched for subm (the output indices are the input's)
 *   nbr            [out_cap, K] int32, K = prod(kernel) <= 27: input row of offset o, -1 = absent
 *   n_out_dev      device int32: the number of output rows (n_in for subm).  It may exceed out_cap: rows past out_cap are not
 *                  written, and the caller repeats the call with more room; out_cap >= min(n_in * prod(ceil(k / s)), output cells)
 *                  always suffices.  subm needs out_cap >= n_in.  Rows at and behind the count are never written.
 * Keys are ((b D + z) H + y) W + x in int32: a key space (input or output grid, times batch) of 2^31 or more returns LVQ_EOVERFLOW
 * before anything is launched (one scene of 41 x 1440 x 1440 fits; 26 do not).  Every axis is range-checked before a key is formed, so
 * a neighbour across an x, y, z or scene edge reads as absent.  No hash table: the ascending-unique kernels of lvq_voxelize_dynamic rank
 * the cells, neighbours are found by a binary search of at most 32 steps -- every loop has a bound known at launch. */
size_t lvq_sparse_conv_rules_workspace_bytes(int64_t n_in, int ndim, const int32_t *spatial_shape_host, int batch, const int32_t *kernel_host,
                                             const int32_t *stride_host, const int32_t *padding_host, int subm);
int lvq_sparse_conv_rules(const int32_t *indices, int64_t n_in, int ndim, const int32_t *spatial_shape_host, int batch,
                          const int32_t *kernel_host, const int32_t *stride_host, const int32_t *padding_host, int subm, int64_t out_cap,
                          int32_t *out_indices, int32_t *nbr, int32_t *n_out_dev, void *ws, size_t ws_bytes, lvq_stream_t stream);

/* The convolution itself (spconv_backbone_voxelnext.py:8-66: conv + BatchNorm1d + ReLU of post_act_block, conv + bn + residual + relu
 * of SparseBasicBlock) as a gather-form implicit GEMM on bf16 MFMA tiles with fp32 accumulation; semantics above.
 *   lvq_sparse_conv_pack_weights   once per weights version: weight [C_out, K, C_in] fp32 -> w_hi (+ w_lo, or NULL) of
 *                                  lvq_sparse_conv_packed_elems(c_out, k_vol, c_in) bf16 elements each ([K][C_out][C_in padded to 32]).
 *   lvq_sparse_conv                feat [n_in, c_in] fp32, nbr [n_out_cap, k_vol] from lvq_sparse_conv_rules, out [n_out_cap, c_out] fp32.
 *                                  w_lo != NULL: features and weights as hi + lo, three products (bf16x3); NULL: plain bf16 operands.
 *                                  bias / scale + shift (both or neither) / residual [n_out_cap, c_out] may be NULL.  n_out_dev (device
 *                                  int32, may be NULL = all n_out_cap rows; clamped to n_out_cap): rows at and behind it are not written.
 *                                  A table entry outside [0, n_in) reads as absent.  No workspace.
 * c_in in {4, 5, 16, 32, 64, 128} with c_out in {16, 32, 64, 128}, or the wide pairs (c_in, c_out) = (128, 256) and (256, 256); k_vol <= 27;
 * anything else ((256, 128) included) returns LVQ_EUNSUPPORTED.  c_in = 256 is summed as two 128-channel stages per offset, ascending, so the
 * order above holds.  w_hi / w_lo 16-byte aligned, feat 16-byte aligned when c_in % 4 == 0. */
size_t lvq_sparse_conv_packed_elems(int c_out, int k_vol, int c_in);
int lvq_sparse_conv_pack_weights(const float *weight, int c_out, int k_vol, int c_in, lvq_bf16 *w_hi, lvq_bf16 *w_lo, lvq_stream_t stream);
int lvq_sparse_conv(const float *feat, int64_t n_in, int c_in, const int32_t *nbr, int k_vol, int64_t n_out_cap, const int32_t *n_out_dev,
                    const lvq_bf16 *w_hi, const lvq_bf16 *w_lo, int c_out, const float *bias, const float *scale, const float *shift,
                    const float *residual, int relu, float *out, lvq_stream_t stream);

/* The branch convs of VoxelNeXtHead (voxelnext_head.py:13-47; csrc/sparse_head.hip): every branch of every task in ONE launch over the n
 * active rows.  A branch is SubMConv2d(128, 128, k) + BatchNorm1d + ReLU followed by SubMConv2d(128, out, 1, bias).
 *   feat        [n, 128] fp32;  nbr [n, k_vol] int32 from lvq_sparse_conv_rules(subm, 2-D), k_vol = 9, or k_vol = 1 where nbr may be NULL
 *               ("row i reads row i").  An entry outside [0, n) reads as absent.
 *   task_n_br   HOST [n_tasks]: branches of each task (1 .. 8, each <= br_stride);  chan_owner HOST [n_tasks, task_c]: the branch that owns
 *               output channel c of the task, negative = nobody (task_c <= 16; channels task_c .. 15 have no owner either)
 *   w_hi, w_lo  [n_tasks][br_stride][k_vol][128][128] bf16: per (task, branch) exactly what lvq_sparse_conv_pack_weights writes for
 *               (c_out 128, k_vol, c_in 128); w_lo == NULL is the plain form, else hi*hi + hi*lo + lo*hi.  Slots of branches a task
 *               does not have are not read.
 *   scale/shift [n_tasks][br_stride][128] fp32, the folded BatchNorm (a conv bias folded by the caller: shift' = bias * scale + shift)
 *   w_last      [n_tasks][16][128] fp32, bias [n_tasks][16]: output channel c reads the intermediate of the branch that owns c
 *   num_conv    2: as above.  1: there is no first conv, the last conv reads feat itself (nbr, w_hi, w_lo, scale, shift are ignored).
 *   out         CHANNEL-major [16 * n_tasks, n] fp32: channel 16 t + c of row i at (16 t + c) * n + i.  The decode scans hm over all rows
 *               and gathers the box channels of K rows only.  Channels nobody owns are written as zeros.
 * Order: lvq_sparse_conv's -- offsets ascending, channels ascending inside an offset, fp32 accumulation, no atomics; the last conv is an
 * fp32 fmaf chain over the 128 intermediate channels in ascending order, then + bias.  A row's bits depend on its own neighbours only:
 * not on its tile, its position, n or the other scenes.  The 128-wide intermediate stays on chip.
 * c_in != 128, k_vol outside {1, 9}, more than 16 tasks, more than 8 branches or 16 output channels in a task, misaligned (16 bytes)
 * feat / w_hi / w_lo, n >= 2^31: LVQ_EUNSUPPORTED.  NULL operands (nbr with k_vol = 9), non-positive sizes, an owner >= the task's branch
 * count, num_conv outside {1, 2}: LVQ_EINVAL.  Every refusal comes before any launch; no allocation, no workspace, stream-ordered. */
int lvq_sparse_head(const float *feat, int64_t n, int c_in, const int32_t *nbr, int k_vol, int n_tasks, const int32_t *task_n_br, int br_stride,
                    const int32_t *chan_owner, int task_c, int num_conv, const lvq_bf16 *w_hi, const lvq_bf16 *w_lo, const float *scale,
                    const float *shift, const float *w_last, const float *bias, float *out, lvq_stream_t stream);

/* =====================================================================================
 * Dense 2-D BEV backbone (csrc/conv2d.hip): the layers of BaseBEVBackbone / BaseBEVBackboneV1 and of PillarRes18BackBone8x's dense conv5
 * ===================================================================================== */

/* Semantics (torch.nn.Conv2d / ConvTranspose2d / eval BatchNorm2d / ReLU as pcdet/models/backbones_2d/base_bev_backbone.py:6-204 stacks them).
 *   planes    an activation is channels-last 16-bit operand planes [B, H, W, Cp] bf16, Cp = C rounded up to a multiple of 32 (zeros beyond
 *             C): a hi plane and, for the bf16x3 form, a lo plane with hi + lo ~ the fp32 value.  lvq_conv2d_to_planes makes them from the
 *             reference's [B, C, H, W] fp32 `spatial_features`; every conv writes the next conv's planes from its epilogue.
 *   conv      cross-correlation, weight torch's [C_out, C_in, k, k]:  kernel 3, padding 1, stride 1 or 2 (output floor((H - 1) / s) + 1
 *             per axis), or kernel = stride = s in {1, 2, 4}, padding 0 (output floor(H / s)).  lvq_conv2d_out_size is that rule.
 *   deconv    ConvTranspose2d(kernel = stride = s), s in {1, 2, 4}, weight torch's [C_in, C_out, s, s]:
 *             out[b, co, s y + i, s x + j] = sum_ci in[b, ci, y, x] W[ci, co, i, j]  (a GEMM with s^2 C_out columns + a pixel shuffle).
 *   epilogue  y = [relu](acc * scale[co] + shift[co]); scale / shift both or neither (NULL = identity).  lvq_conv2d_res adds a residual.
 *   outputs   out_hi (+ out_lo) planes [B, OH, OW, out_c_total] and / or out_f32 [B, out_c_total, OH, OW] fp32 (the reference's
 *             `spatial_features_2d` layout); at least one.  The layer writes channels out_c_off .. out_c_off + c_out - 1 of either and
 *             nothing else: deblocks write straight into their range of the concatenated result.
 *   forms     w_lo != NULL: hi + lo operands, three products (bf16x3), in_lo required; w_lo == NULL: plain bf16, in_lo must be NULL.
 *   order     32-channel chunks ascending, taps (ky * k + kx) ascending inside a chunk of the staged tile, fp32 accumulation, no atomics:
 *             a pixel's bits depend on its own receptive field only, not on its position, tile, scene or the canvas size.
 * Family: c_in 1 .. 512 (the input planes hold c_in rounded up to 32 channels), c_out a multiple of 64 in 64 .. 512, batch <= 65535;
 * a (kernel, stride) or channel count outside it returns LVQ_EUNSUPPORTED, an inconsistent call (non-positive size, NULL operand, one of
 * scale / shift, in_lo without w_lo, out_c_off + c_out > out_c_total, a kernel = stride larger than the canvas) LVQ_EINVAL; both before
 * any launch.  Plane and packed-weight pointers are 16-byte aligned.  No workspace, no allocation, stream-ordered.
 *   lvq_conv2d_plane_elems     batch * h * w * (c rounded up to 32), 0 outside the family                              (host only)
 *   lvq_conv2d_out_size        output size of one axis, or the negative error code                                     (host only)
 *   lvq_conv2d_packed_elems    (c_in rounded up to 32) * kernel^2 * c_out bf16 elements per part, 0 outside the family (host only;
 *                              transposed != 0: kernel is the stride s of the transposed conv)
 *   lvq_conv2d_pack_weights    once per weights version: fp32 weight -> w_hi (+ w_lo, or NULL) in MFMA-fragment order
 *   lvq_conv2d_res             lvq_conv2d with a residual operand (the dense BasicBlock of spconv_backbone_2d.py:79-111): res_hi (+ res_lo)
 *                              are planes [B, OH, OW, c_out], the layout of this layer's own output planes without a channel offset, and
 *                              y = [relu](acc * scale + shift + res), res = hi + lo in the bf16x3 form (res_lo may be NULL = hi alone), res =
 *                              hi in the plain form.  A conv bias is folded by the caller: shift' = bias * scale + shift.  res_hi == NULL,
 *                              res_lo in the plain form (w_lo == NULL) and planes that are not 16-byte aligned follow the rules above
 *                              (LVQ_EINVAL / LVQ_EINVAL / LVQ_EUNSUPPORTED), before any launch. */
size_t lvq_conv2d_plane_elems(int batch, int c, int h, int w);
int lvq_conv2d_out_size(int in, int kernel, int stride);
int lvq_conv2d_to_planes(const float *x, int batch, int c, int h, int w, lvq_bf16 *hi, lvq_bf16 *lo, lvq_stream_t stream);
size_t lvq_conv2d_packed_elems(int c_out, int c_in, int kernel, int transposed);
int lvq_conv2d_pack_weights(const float *weight, int c_out, int c_in, int kernel, int transposed, lvq_bf16 *w_hi, lvq_bf16 *w_lo,
                            lvq_stream_t stream);
int lvq_conv2d(const lvq_bf16 *in_hi, const lvq_bf16 *in_lo, int batch, int h, int w, int c_in, const lvq_bf16 *w_hi, const lvq_bf16 *w_lo,
               int c_out, int kernel, int stride, const float *scale, const float *shift, int relu, lvq_bf16 *out_hi, lvq_bf16 *out_lo,
               float *out_f32, int out_c_total, int out_c_off, lvq_stream_t stream);
int lvq_conv2d_res(const lvq_bf16 *in_hi, const lvq_bf16 *in_lo, int batch, int h, int w, int c_in, const lvq_bf16 *w_hi, const lvq_bf16 *w_lo,
                   int c_out, int kernel, int stride, const float *scale, const float *shift, const lvq_bf16 *res_hi, const lvq_bf16 *res_lo,
                   int relu, lvq_bf16 *out_hi, lvq_bf16 *out_lo, float *out_f32, int out_c_total, int out_c_off, lvq_stream_t stream);
int lvq_deconv2d(const lvq_bf16 *in_hi, const lvq_bf16 *in_lo, int batch, int h, int w, int c_in, const lvq_bf16 *w_hi, const lvq_bf16 *w_lo,
                 int c_out, int stride, const float *scale, const float *shift, int relu, lvq_bf16 *out_hi, lvq_bf16 *out_lo, float *out_f32,
                 int out_c_total, int out_c_off, lvq_stream_t stream);

/* =====================================================================================
 * CenterHead post-processing (csrc/center_head.hip): heat maps -> box candidates -> rotated BEV NMS -> per-scene lists
 * ===================================================================================== */

/* Top-K + decode of centernet_utils.py:155-241 as center_head.py:297-326 calls it, for every (scene, task) in ONE launch.
 *   maps          [batch, c_total, h, w] fp32: the raw outputs of the tasks' last convs, all tasks side by side in the channels
 *   task_channels HOST [n_tasks, 6] int32: first channel of center (2), center_z (1), dim (3), rot (2: cos, sin), vel (2, or -1 = none)
 *                 and hm (n_cls) of each task;  task_n_cls HOST [n_tasks];  class_map HOST [sum n_cls]: the tasks' class-id mappings
 *                 one behind the other (center_head.py:329).  All three are copied into the kernel's arguments: at most 16 tasks and
 *                 64 classes in all (else LVQ_EUNSUPPORTED).
 *   per group g = scene * n_tasks + task: the k largest sigmoid(hm) over n_cls * h * w (class = flat index / (h * w)), descending,
 *                 EQUAL SCORES TOWARDS THE LOWER FLAT INDEX; dim = exp, heading = atan2(sin, cos), x = (col + center_x) * stride *
 *                 voxel_xy[0] + range_xy[0] (y alike with the row), each product rounded to fp32 in that order; a candidate stays when
 *                 limit_range[0..2] <= (x, y, z) <= limit_range[3..5] and score > score_thresh (a negative score_thresh keeps every
 *                 score: the reference's None); the survivors are compacted in score order.
 *   outputs       boxes [batch, n_tasks, k, box_dim] fp32 (box_dim 9 = with vel in every task, 7 = in none), scores [batch, n_tasks, k],
 *                 labels [batch, n_tasks, k] int32 (mapped, 0-based), counts [batch, n_tasks] int32; rows behind a count are zeros.
 * k <= 1024 (else LVQ_EUNSUPPORTED); k > n_cls * h * w of any task: LVQ_EINVAL (torch.topk raises there), as are NULL operands, non-positive
 * sizes, a channel range outside c_total and a box_dim that disagrees with the vel channels.  ws below the query: LVQ_EWORKSPACE.  Every
 * refusal happens before any launch.  One workgroup per group, nothing handed between workgroups; no allocation, stream-ordered.
 * The query writes *bytes and returns a status like every call (max_cls = the largest n_cls of a task). */
int lvq_center_decode_workspace_bytes(int batch, int n_tasks, int max_cls, int h, int w, size_t *bytes);
int lvq_center_decode(const float *maps, int batch, int c_total, int h, int w, int n_tasks, const int32_t *task_channels,
                      const int32_t *task_n_cls, const int32_t *class_map, int k, int box_dim, int stride, const float *voxel_xy,
                      const float *range_xy, const float *limit_range, float score_thresh, float *boxes, float *scores, int32_t *labels,
                      int32_t *counts, void *ws, size_t ws_bytes, lvq_stream_t stream);

/* Pairwise rotated BEV IoU of iou3d_nms_utils.py:31-45: boxes_a [n, 7], boxes_b [m, 7] fp32 rows (x, y, z, dx, dy, dz, heading), dx, dy > 0;
 * iou [n, m] fp32 = area(a ^ b) / max(dx_a dy_a + dx_b dy_b - area, 1e-8).  The area is the exact intersection of the two rotated
 * rectangles (a's corners in b's frame, clipped against b's four sides, shoelace), in fp32: no corner margin.  One launch, no workspace.
 * NULL operand or non-positive count: LVQ_EINVAL; n above 262140: LVQ_EUNSUPPORTED. */
int lvq_boxes_iou_bev(const float *boxes_a, int n, const float *boxes_b, int m, float *iou, lvq_stream_t stream);

/* nms_gpu of iou3d_nms_utils.py:120-135 under class_agnostic_nms (model_nms_utils.py:6-25) for `groups` independent lists in two launches
 * and no host round trip.  boxes [groups, n_max, box_stride] fp32, box_stride >= 7 (the first seven floats of a row are used), each
 * group ALREADY in descending score order; counts [groups] int32 on the DEVICE, read by the kernels only, clamped to 0 .. n_max.
 *   n = min(counts[g], pre_max) rows enter (NMS_PRE_MAXSIZE truncates before NMS); row j is dropped when a kept row i < j has
 *   iou(i, j) > thresh (strict); keep [groups, post_max] int32 = the kept row numbers ascending, cut at post_max (NMS_POST_MAXSIZE), -1 behind
 *   keep_count [groups].  Launch 1: one wave per 64 x 64 tile on or above the diagonal writes the suppression words into ws; launch 2:
 *   one wave per group walks them.  The IoU is lvq_boxes_iou_bev's.
 * n_max <= 1024 and groups <= 65535 (else LVQ_EUNSUPPORTED); NULL operand, non-positive size, box_stride < 7: LVQ_EINVAL; ws below the
 * query: LVQ_EWORKSPACE; all before any launch.  The query writes *bytes and returns a status. */
int lvq_nms_bev_workspace_bytes(int groups, int n_max, size_t *bytes);
int lvq_nms_bev(const float *boxes, int box_stride, const int32_t *counts, int groups, int n_max, int pre_max, int post_max, float thresh,
                int32_t *keep, int32_t *keep_count, void *ws, size_t ws_bytes, lvq_stream_t stream);

/* The gather and concatenation of center_head.py:352-363 in one launch: for scene b the kept rows of task 0, then of task 1, ... go to
 * out_boxes [batch, n_tasks * post_max, box_dim], out_scores [batch, n_tasks * post_max] and out_labels [batch, n_tasks * post_max] int64
 * (labels + 1: 1-based); out_count [batch] int32 = the scene's total.  boxes / scores / labels are lvq_center_decode's outputs with k
 * rows per group, keep / keep_count lvq_nms_bev's with groups = batch * n_tasks.  Rows behind out_count are left as they were: the caller
 * slices.  n_tasks <= 16 (else LVQ_EUNSUPPORTED); NULL operand, non-positive size, box_dim outside {7, 9}: LVQ_EINVAL, before the launch. */
int lvq_center_collect(const float *boxes, const float *scores, const int32_t *labels, const int32_t *keep, const int32_t *keep_count,
                       int batch, int n_tasks, int k, int box_dim, int post_max, float *out_boxes, float *out_scores, int64_t *out_labels,
                       int32_t *out_count, lvq_stream_t stream);

/* Top-K + decode of centernet_utils.py:243-354 (decode_bbox_from_voxels_nuscenes, as voxelnext_head.py:443-456 calls it) over the rows of
 * a sparse tensor, for every (scene, task) in ONE launch.  The selection, the sort, the masks and the compaction are lvq_center_decode's.
 *   head          CHANNEL-major [c_total, n_rows] fp32: lvq_sparse_head's output (c_total = 16 * n_tasks there)
 *   indices       [n_rows, 3] int32 (b, y, x).  The candidates of a scene are the rows with b == scene, in stored order; they need not be
 *                 contiguous.  A row whose b is outside [0, batch) takes no part.
 *   task_channels / task_n_cls / class_map, k, box_dim, stride, voxel_xy, range_xy, limit_range, score_thresh: as for lvq_center_decode.
 *   per group g = scene * n_tasks + task: the min(k, n_cls * n_b) largest sigmoid(hm) of the scene's n_b rows, descending, EQUAL SCORES
 *                 TOWARDS THE LOWER (class, stored row) PAIR (the lower flat index of the reference's [n_cls, n_b] matrix); NaNs first;
 *                 dim = exp, heading = atan2(sin, cos), x = (col + center_x) * stride * voxel_xy[0] + range_xy[0] (y alike with the row),
 *                 each product rounded to fp32 in that order; limit-range and score masks; compaction in score order.
 *   outputs       exactly lvq_center_decode's: boxes [batch, n_tasks, k, box_dim], scores, labels int32 (mapped, 0-based), counts
 *                 [batch, n_tasks]; rows behind a count are zeros.  lvq_nms_bev and lvq_center_collect take them unchanged.
 * ONE DELIBERATE DIFFERENCE from the reference: when a scene has fewer than k rows, _topk_1d still computes class = ind // k on an
 * [n_cls, n_b] matrix, which gives wrong classes, and when n_cls * n_b < k its torch.stack / .view(batch, k) raise.  Here the class is the
 * matrix row the candidate came from and the count is what there is (a scene without rows: count 0, no row is read).  With n_b >= k in
 * every scene the two agree.
 * k <= 1024, at most 16 tasks and 64 classes, max_cls * n_rows < 2^31 (else LVQ_EUNSUPPORTED); NULL operands, non-positive batch or k, a
 * channel range outside c_total, a box_dim that disagrees with the vel channels: LVQ_EINVAL; ws below the query: LVQ_EWORKSPACE.  Every
 * refusal happens before the launch.  One workgroup per group, nothing handed between workgroups; no allocation, stream-ordered. */
int lvq_voxel_decode_workspace_bytes(int batch, int n_tasks, int max_cls, int64_t n_rows, size_t *bytes);
int lvq_voxel_decode(const float *head, const int32_t *indices, int64_t n_rows, int batch, int c_total, int n_tasks,
                     const int32_t *task_channels, const int32_t *task_n_cls, const int32_t *class_map, int k, int box_dim, int stride,
                     const float *voxel_xy, const float *range_xy, const float *limit_range, float score_thresh, float *boxes, float *scores,
                     int32_t *labels, int32_t *counts, void *ws, size_t ws_bytes, lvq_stream_t stream);

/* =====================================================================================
 * AnchorHeadSingle (csrc/anchor_head.hip): head maps -> a box for every anchor -> the NMS_PRE_MAXSIZE best -> rotated BEV NMS of up to 4096 rows
 * ===================================================================================== */

/* generate_predicted_boxes of anchor_head_template.py:225-272 for EVERY anchor of every scene in ONE launch.
 *   maps          [batch, c_total, h, w] fp32: the raw outputs of conv_cls, conv_box and conv_dir_cls side by side in the channels.
 *                 cls_channel / box_channel / dir_channel: the first channel of each (dir_channel -1 = no direction classifier); anchor a
 *                 of a pixel reads channels cls_channel + a * n_cls + k, box_channel + a * 7 + d and dir_channel + a * n_dir_bins + j.
 *   anchors       [h * w * n_anchors, 7] fp32 on the DEVICE in the reference's flat order (y, x, a): (xa, ya, za, dxa, dya, dza, ra)
 *   per anchor n = (y * w + x) * n_anchors + a, each step rounded to fp32 in this order (ResidualCoder.decode_torch, box_coder_utils.py:45-80):
 *                 diag = sqrt(dxa^2 + dya^2); x = xt * diag + xa, y alike; z = zt * dza + za; d* = exp(d*t) * d*a; r = rt + ra.  With a
 *                 direction classifier: bin = argmax over the bins (ties to the lower bin), v = r - dir_offset, period = 2 pi /
 *                 n_dir_bins rounded to fp32, r = v - floor(v / period + dir_limit_offset) * period + dir_offset + period * bin.
 *                 score = max_k sigmoid(logit_k), label = the lowest k that attains it; a NaN logit gives a NaN score.
 *   outputs       cls_preds [batch, N, n_cls] (the raw logits, regrouped), box_preds [batch, N, 7], scores [batch, N], labels [batch, N]
 *                 int32 (0-based), N = h * w * n_anchors.
 *   cand / cand_count   both NULL, or cand [batch, N] int32 and cand_count [batch] int32 (zeroed by the call): the anchors with score >=
 *                 score_thresh (inclusive, model_nms_utils.py:9; a NaN fails it) as a SET: cand[b, 0 .. cand_count[b] - 1] hold their
 *                 indices n in NO PARTICULAR ORDER, which may differ from run to run.  lvq_anchor_select does not depend on it.
 * n_cls <= 64, N < 2^31, batch <= 65535, n_anchors * (n_cls + 10) <= 12284 (a pixel's anchors fit 48 KB of LDS) (else LVQ_EUNSUPPORTED);
 * NULL operands, non-positive sizes, a channel range outside c_total, one of cand / cand_count without the other: LVQ_EINVAL.  Every
 * refusal happens before the launch.  No workspace, no allocation, stream-ordered. */
int lvq_anchor_decode(const float *maps, int batch, int c_total, int h, int w, int cls_channel, int box_channel, int dir_channel,
                      int n_anchors, int n_cls, int n_dir_bins, float dir_offset, float dir_limit_offset, const float *anchors,
                      float score_thresh, float *cls_preds, float *box_preds, float *scores, int32_t *labels, int32_t *cand,
                      int32_t *cand_count, lvq_stream_t stream);

/* class_agnostic_nms of model_nms_utils.py:6-25 up to the NMS call, for every scene in ONE launch (one workgroup per scene).
 *   scores [batch, n], labels [batch, n] int32, box_preds [batch, n, 7]: lvq_anchor_decode's outputs (or the same made elsewhere)
 *   candidates    has_thresh != 0: the anchors with score >= score_thresh (a NaN fails it); has_thresh == 0 (SCORE_THRESH None): all
 *                 anchors, and a NaN of either sign sorts first, as torch.topk has it.
 *   per scene     the min(pre_max, candidates) largest scores, descending, EQUAL SCORES TOWARDS THE LOWER ANCHOR INDEX (-0.0 and +0.0
 *                 are equal scores: between them the index decides, as `>=` and torch.topk compare them; any sign is accepted):
 *                 sel_boxes [batch, pre_max, 7], sel_scores [batch, pre_max], sel_labels [batch, pre_max] int32 (as given, 0-based),
 *                 sel_index [batch, pre_max] int32 (the anchor index), sel_count [batch] int32; rows behind a count are zeros with
 *                 index -1.  lvq_nms_bev_wide and lvq_center_collect (n_tasks 1, k = pre_max) take them unchanged.
 *   cand / cand_count   both NULL: the kernel scans all n scores.  Otherwise lvq_anchor_decode's candidate set for the SAME score_thresh
 *                 (has_thresh must be set): only the list is read; an entry outside 0 .. n - 1 or below the threshold takes no part.
 *                 The two routes return identical outputs, whatever the order of the list.
 * pre_max <= 4096 (the sort's 32 KB of LDS), n < 2^31, batch <= 65535 (else LVQ_EUNSUPPORTED); NULL operands, non-positive sizes, a list
 * without has_thresh: LVQ_EINVAL; ws below the query: LVQ_EWORKSPACE; all before the launch.  The query writes *bytes and returns a status. */
int lvq_anchor_select_workspace_bytes(int batch, int64_t n, size_t *bytes);
int lvq_anchor_select(const float *scores, const int32_t *labels, const float *box_preds, int batch, int64_t n, int has_thresh,
                      float score_thresh, int pre_max, const int32_t *cand, const int32_t *cand_count, float *sel_boxes, float *sel_scores,
                      int32_t *sel_labels, int32_t *sel_index, int32_t *sel_count, void *ws, size_t ws_bytes, lvq_stream_t stream);

/* lvq_nms_bev for lists of up to 4096 rows (NMS_PRE_MAXSIZE of the anchor heads): the same semantics, outputs, workspace rule and
 * refusals, with n_max <= 4096.  The same two kernels: up to 64 x 64 mask tiles per group, and a walk that keeps a [64][64] word tile
 * in LDS (lane w holds word w of the removed set, so 64 words are what one wave walks).  For n_max <= 1024 the keep lists equal
 * lvq_nms_bev's. */
int lvq_nms_bev_wide_workspace_bytes(int groups, int n_max, size_t *bytes);
int lvq_nms_bev_wide(const float *boxes, int box_stride, const int32_t *counts, int groups, int n_max, int pre_max, int post_max, float thresh,
                     int32_t *keep, int32_t *keep_count, void *ws, size_t ws_bytes, lvq_stream_t stream);

/* =====================================================================================
 * TransFusionHead (csrc/transfusion_head.hip): heat-map proposals -> object queries -> (decoder layer on lvq_gemm_bf16 / lvq_attention_bf16 /
 * lvq_layernorm) -> feed-forward, prediction branches and box decode
 * ===================================================================================== */

/* The query initialisation of transfusion_head.py:161-185 for every scene in ONE launch (one workgroup per scene).
 *   maps          [batch, c_total, h, w] fp32: the raw heat-map logits are channels first_channel .. first_channel + n_cls - 1
 *   heat          sigmoid(logit).  A cell of a class survives when heat == the maximum over its 3 x 3 neighbourhood, compared in the sigmoid
 *                 domain (a plateau keeps all its equal cells); a border cell never survives (the reference's local_max is zero there).
 *                 A class whose bit is set in point_class_mask keeps every cell, border included (nuScenes: classes 8, 9; Waymo: 1, 2).
 *                 A cell that does not survive scores exactly 0.  A NaN heat stays NaN; a cell with a NaN neighbour does not survive.
 *   outputs       per scene the n_proposals largest of the n_cls * h * w values, descending, EQUAL VALUES TOWARDS THE LOWER FLAT INDEX (the
 *                 reference's argsort leaves ties open), NaN first: prop_flat [batch, n_proposals] int32 (class = flat / (h w), cell =
 *                 flat % (h w)), prop_score [batch, n_proposals], and query_heatmap_score [batch, n_cls, n_proposals], the surviving heat
 *                 of EVERY class at the chosen cell (transfusion_head.py:212-215).
 * n_proposals <= 1024 and nms_kernel_size == 3 (else LVQ_EUNSUPPORTED); n_proposals > n_cls * h * w, h or w < 3, n_cls > 64, NULL
 * operands, non-positive sizes, a channel range outside c_total: LVQ_EINVAL; ws below the query: LVQ_EWORKSPACE.  Every refusal happens
 * before the launch, outputs untouched.  No allocation, stream-ordered; a scene's outputs do not depend on the other scenes. */
int lvq_heatmap_proposals_workspace_bytes(int batch, int n_cls, int h, int w, size_t *bytes);
int lvq_heatmap_proposals(const float *maps, int batch, int c_total, int h, int w, int first_channel, int n_cls,
                          int64_t point_class_mask, int nms_kernel_size, int n_proposals, int32_t *prop_flat, float *prop_score,
                          float *query_heatmap_score, void *ws, size_t ws_bytes, lvq_stream_t stream);

/* PositionEmbeddingLearned of transfusion_utils.py:10-26 in eval(): pos [n, 2] fp32 -> out [n, d_out] fp32,
 *   out = W2 relu((W1 pos) * scale + shift) + b2,   W1 [d, 2], W2 [d_out, d] (Conv1d weights without their last axis), b2 [d_out];
 *   scale / shift [d]: the BatchNorm1d folded by the caller with the first conv's bias, shift = b1 * scale + (beta - mean * scale).
 * The module itself has d_out = d.  A caller that feeds the embedding to a Linear alone may fold that Linear into W2 / b2 (TransFusionHead's
 * key table through the K | V projection: d_out = 2 d), so the table of every grid cell comes out of this one launch.
 * fp32 operands and FMA accumulation in ascending k; a row's bits do not depend on its position or on n.  d a multiple of 4, d and d_out up
 * to 512, W2 16-byte aligned (else LVQ_EUNSUPPORTED); NULL operands, n, d or d_out <= 0: LVQ_EINVAL; before the launch.  No workspace. */
int lvq_pos_embed_learned(const float *pos, int64_t n, int d, int d_out, const float *w1, const float *scale, const float *shift, const float *w2,
                          const float *b2, float *out, lvq_stream_t stream);

/* The object queries of transfusion_head.py:186-204 for lvq_heatmap_proposals' prop_flat, in two launches.
 *   feat_hi / feat_lo   the shared conv's output planes [batch, h, w, d] bf16 (lvq_conv2d); feat_lo NULL: the plain form, hi alone
 *   query_feat    [batch, n_proposals, d] fp32 = (hi + lo)[cell] + (class_w[:, class] + class_b): the one-hot Conv1d of class_encoding is a
 *                 column pick; class_w [d, n_cls], class_b [d]
 *   query_pos     [batch, n_proposals, 2] fp32 = (cell % y_size + 0.5, cell / y_size + 0.5): THE REFERENCE'S OWN FORMULA -- create_2D_grid
 *                 (transfusion_head.py:125-135) is an `ij` meshgrid over (x_size, y_size) that predict() indexes with the row-major cell
 *                 and flips.  On a square grid that is (column + 0.5, row + 0.5); on any other it is not, and it is reproduced as it is.
 *   query_labels  [batch, n_proposals] int32 = flat / (h w)
 *   query_pe      [batch, n_proposals, d] fp32 = lvq_pos_embed_learned(query_pos) with the pe_* operands (self_posembed)
 * d a multiple of 32 up to 512, n_cls <= 64 (else LVQ_EUNSUPPORTED); NULL operands, non-positive sizes: LVQ_EINVAL; before any launch.  An
 * entry of prop_flat outside 0 .. n_cls h w - 1 is clamped into it, never used as it is. */
int lvq_transfusion_queries(const lvq_bf16 *feat_hi, const lvq_bf16 *feat_lo, int batch, int h, int w, int d, const int32_t *prop_flat,
                            int n_proposals, int n_cls, int y_size, const float *class_w, const float *class_b, const float *pe_w1,
                            const float *pe_scale, const float *pe_shift, const float *pe_w2, const float *pe_b2, float *query_feat,
                            float *query_pos, int32_t *query_labels, float *query_pe, lvq_stream_t stream);

/* with_pos_embed of transfusion_utils.py:64-65 as a GEMM operand: hi (+ lo, or NULL) = bf16 parts of x + pe, n elements each. */
int lvq_transfusion_add_pe(const float *x, const float *pe, int64_t n, lvq_bf16 *hi, lvq_bf16 *lo, lvq_stream_t stream);

/* The rest of the decoder layer and the head for the batch * n_proposals query rows (transfusion_utils.py:95-97; transfusion_head.py:15-49,
 * 209-210, 397-479), fp32 operands and FMA accumulation in ascending k throughout (no bf16 rounding: the bits do not depend on a precision mode).
 *   x             [batch, n_proposals, 128] fp32: the output of norm2
 *   ffn           y = norm3(x + W2 relu(W1 x + b1) + b2): w1 [ffn, 128], w2 [128, ffn], gamma / beta [128], centred statistics
 *   branches      center (2), height (1), dim (3), rot (2), vel (2, with has_vel), heatmap (n_cls), in this order: head_w1 [nb * 64, 128]
 *                 with head_scale / head_shift [nb * 64] (the folded BatchNorm1d and conv bias) and ReLU; head_w2 [c_total, 64] whose row o
 *                 reads the 64 features of o's branch, head_b2 [c_total]; c_total = (has_vel ? 10 : 8) + n_cls
 *   raw           [batch, c_total, n_proposals] fp32, the reference's res_layer channel-major; `center` already carries + query_pos
 *   decode        score = sigmoid(heatmap[label]) * prop_score, label = query_labels (the reference takes the argmax of a product with a
 *                 one-hot, which is the query's class whenever the score is not 0); x = (center_x * stride) * voxel_xy[0] + range_xy[0] (y
 *                 alike), each product rounded to fp32 in that order; dim = exp; heading = atan2(rot[0], rot[1]) -- channel 0 is the SINE;
 *                 a row stays when score > score_thresh (strict) and limit_range[0..2] <= (x, y, z) <= limit_range[3..5]
 *   outputs       boxes [batch, n_proposals, 9 or 7], scores, labels int32 (query class + 1), counts [batch] int32: the kept rows IN
 *                 PROPOSAL ORDER, zeros behind a count.  voxel_xy / range_xy / limit_range are HOST arrays.
 * Two launches: 8 rows per workgroup, then one workgroup per scene for the order-keeping compaction (a row's rank is a prefix over its
 * scene).  n_proposals <= 1024, ffn a multiple of 64 up to 512, n_cls <= 64, 16-byte aligned weights (else LVQ_EUNSUPPORTED); NULL
 * operands, non-positive sizes: LVQ_EINVAL; ws below the query: LVQ_EWORKSPACE; all before any launch, outputs untouched. */
int lvq_transfusion_tail_workspace_bytes(int batch, int n_proposals, int box_dim, size_t *bytes);
int lvq_transfusion_tail(const float *x, const float *query_pos, const int32_t *query_labels, const float *prop_score, int batch,
                         int n_proposals, int ffn, int n_cls, int has_vel, const float *w1, const float *b1, const float *w2, const float *b2,
                         const float *gamma, const float *beta, float eps, const float *head_w1, const float *head_scale,
                         const float *head_shift, const float *head_w2, const float *head_b2, int stride, const float *voxel_xy,
                         const float *range_xy, const float *limit_range, float score_thresh, float *raw, float *boxes, float *scores,
                         int32_t *labels, int32_t *counts, void *ws, size_t ws_bytes, lvq_stream_t stream);

/* =====================================================================================
 * Decode-step runtime
 * ===================================================================================== */

/* One greedy-decoding step of the Qwen2-architecture decoder (inference_engine.py:283-296 -> transformers generate with a KV
 * cache) as ONE native call: per layer RMSNorm -> packed q|k|v projection (+bias) -> rotary embedding at position `pos` ->
 * append K, V to the caches -> attention of the one new query over positions 0..pos -> o_proj + residual -> RMSNorm ->
 * gate|up projection -> SiLU(gate)*up -> down projection + residual.  The same kernels, order and arguments as the
 * Python loop of head.StandInHead (bit-identical), without ~14 ctypes round trips per layer.
 *   x [batch, d] fp32: embedding of the new token in, hidden state out (final norm + lm head are the caller's)
 *   layers: HOST array of n_layers structs of DEVICE pointers; weights are bf16 (hi) with optional lo parts (precision 3)
 *   caches [batch, lmax, dkv] bf16 (post-rotary keys); pos < lmax; precision: 1 = bf16, 3 = bf16x3 */
/* (decode loop of inference_engine.py:283-296 -> transformers generate with a KV cache, one token per step)
 * RMSNorm fused into a skinny projection (m <= 8 rows): C = (RMSNorm(x) * gamma rounded to bf16[, lo]) @ W^T (+ bias); the
 * rounding and summation order are lvq_rmsnorm's, so the result is bit-identical to lvq_rmsnorm + lvq_gemm_bf16. */
int lvq_gemv_rmsnorm_bf16(const float *x, const float *gamma, float eps, const lvq_bf16 *w, const lvq_bf16 *w_lo, const float *bias,
                          int m, int n, int k, int64_t ldw, int64_t ldc, float *c_f32, lvq_bf16 *c_bf16, lvq_bf16 *c_lo,
                          lvq_stream_t stream);

typedef struct {
    const float *ln1, *ln2;                       /* input_layernorm / post_attention_layernorm weights [d] */
    const lvq_bf16 *wqkv, *wqkv_lo;               /* [d + 2 dkv, d]  (q_proj | k_proj | v_proj rows) */
    const float *bqkv;                            /* [d + 2 dkv] */
    const lvq_bf16 *wo, *wo_lo;                   /* [d, d] */
    const lvq_bf16 *wgu, *wgu_lo;                 /* [2 inter, d]    (gate_proj | up_proj rows) */
    const lvq_bf16 *wdown, *wdown_lo;             /* [d, inter] */
    lvq_bf16 *k_cache, *k_cache_lo, *v_cache, *v_cache_lo;
} lvq_qwen2_layer;
/* one decode step of every layer (inference_engine.py:283-296 -> transformers generate, one new token against the KV cache): contract above */
size_t lvq_qwen2_decode_workspace_bytes(int batch, int d, int n_heads, int n_kv_heads, int inter, int lmax, int precision);
int lvq_qwen2_decode_step(const lvq_qwen2_layer *layers, int n_layers, float *x, int batch, int d, int n_heads, int n_kv_heads,
                          int inter, int pos, int lmax, float rms_eps, float rope_theta, int precision, void *ws, size_t ws_bytes,
                          lvq_stream_t stream);

/* ---- Ragged decode (csrc/decode_ragged.hip): a batch whose sequences stand at different positions ----------------------------
 * Decode attention of inference_engine.py:283-296 -> transformers generate with a KV cache, for a batch of prompts of different
 * length: ONE query token per sequence over the first kv_len[b] rows of its cache,
 *   O[b,h,:] = softmax_j( Q[b,h,:].K[b,j,h/g,:] * scale ) V[b,j,h/g,:],   j < kv_len[b],   g = n_heads / n_kv_heads <= 16.
 *   q rows [batch, n_heads * dh], caches [batch, lmax, n_kv_heads * dh], o [batch, n_heads * dh] (bf16 hi, optional lo), addressed with
 *   the strides of lvq_attention_bf16 (ldq / ldo are accepted and unused: there is one query row); operand strides are multiples
 *   of 8 elements and operand pointers 16-byte aligned.  kv_len [batch] int32 on the DEVICE, read by the kernels only (no host read,
 *   no synchronisation); values are clamped to 0 .. lmax, a length of 0 writes zeros, cache rows at and beyond kv_len[b] are
 *   never loaded.  q_lo != NULL selects hi + lo operands (then k_cache_lo and v_cache_lo are required), the bf16x3 mode of
 *   lvq_attention_bf16; otherwise plain bf16.  dh multiple of 16, <= 128; scale > 0.
 * The query heads of one KV head are the columns of one MFMA tile, so a cache row is loaded once per KV head.  The work of sequence b
 * (fixed-length key chunks, merged in ascending order) depends on kv_len[b] alone: its output bits do not depend on the batch. */
size_t lvq_attention_decode_ragged_workspace_bytes(int batch, int n_heads, int n_kv_heads, int lmax, int dh, int precision);
int lvq_attention_decode_ragged(const lvq_bf16 *q, const lvq_bf16 *q_lo, const lvq_bf16 *k_cache, const lvq_bf16 *k_cache_lo,
                                const lvq_bf16 *v_cache, const lvq_bf16 *v_cache_lo, const int32_t *kv_len, int batch, int n_heads,
                                int n_kv_heads, int lmax, int dh, int64_t q_bstride, int64_t ldq, int64_t q_hstride, int64_t k_bstride,
                                int64_t ldk, int64_t k_hstride, int64_t v_bstride, int64_t ldv, int64_t v_hstride, int64_t o_bstride,
                                int64_t ldo, int64_t o_hstride, float scale, lvq_bf16 *o, lvq_bf16 *o_lo, void *ws, size_t ws_bytes,
                                lvq_stream_t stream);
/* lvq_qwen2_decode_step for a ragged batch (inference_engine.py:283-296 -> transformers generate with a KV cache, prompts of different length):
 * the new token of sequence b sits at position pos0[b] + t and attends keys 0 .. pos0[b] + t.  pos0 [batch] int32 on the DEVICE, never
 * written: a decode loop passes the prompt lengths once and t = 0, 1, ...  0 <= t < lmax is checked on the host; a sequence with
 * pos0[b] + t >= lmax is clamped on the device to position lmax - 1 (it keeps overwriting its last cache row -- its output is then
 * meaningless, but nothing is written outside its cache).  Same projections, norms and SwiGLU calls as lvq_qwen2_decode_step; at
 * equal positions the appended cache rows have equal bits.  Head geometries of lvq_attention_decode_ragged only (else LVQ_EINVAL). */
size_t lvq_qwen2_decode_ragged_workspace_bytes(int batch, int d, int n_heads, int n_kv_heads, int inter, int lmax, int precision);
int lvq_qwen2_decode_step_ragged(const lvq_qwen2_layer *layers, int n_layers, float *x, int batch, int d, int n_heads, int n_kv_heads,
                                 int inter, const int32_t *pos0, int t, int lmax, float rms_eps, float rope_theta, int precision,
                                 void *ws, size_t ws_bytes, lvq_stream_t stream);

/* ---- Shared-prefix decode (csrc/decode_shared.hip): many sequences behind one cached prefix ------------------------------------------
 * The reference's batch mode (infer.py:225-314) answers every question of a scene with its own inference_engine.py:283-296 call, which
 * prefills the same vision / LiDAR prefix again.  Here sequence b continues prefix g = prefix_index[b]: its history is rows
 * 0 .. plen[g]-1 of the prefix caches [n_prefix, pmax, n_kv_heads * dh] followed by the rows of its own caches [batch, lown, n_kv_heads * dh].
 * Nothing is copied: a key at global position p is read from the prefix cache when p < plen[g], else from own row p - plen[g].
 * Sequence b brings qn[b] query rows (q [batch, lq, n_heads * dh]; rows r >= qn[b] are padding and get a zero output) behind own0[b] own
 * rows that are already cached; the keys / values of the query rows themselves are own rows own0[b] .. own0[b] + qn[b] - 1 (the caller
 * has appended them).  Query row r stands at global position plen[g] + own0[b] + r and sees every key up to and including that one:
 *   O[b,r,h,:] = softmax_j( Q[b,r,h,:].K[j,h/g,:] * scale ) V[j,h/g,:],   j <= plen[g] + own0[b] + r.
 * One entry point serves the question prefill (own0 = 0, qn = question length) and a decode step (lq = 1, qn = 1).
 *   prefix_index, own0, qn [batch] and plen [n_prefix]: int32 on the DEVICE, read by the kernels only (no host read, no
 *   synchronisation), clamped to what the buffers hold; rows behind a length are never loaded.  Strides as lvq_attention_bf16 (the
 *   prefix and the own caches share row and head strides and have their own batch strides); operand strides are multiples of 8
 *   elements, operand pointers 16-byte aligned.  q_lo != NULL selects hi + lo operands (then every cache needs its lo part).
 *   dh multiple of 16, <= 128; n_heads / n_kv_heads <= 16; scale > 0.
 * Keys are cut into the fixed 128-key chunks of lvq_attention_decode_ragged at GLOBAL positions and the columns of the MFMA tile are
 * (query row, query head) pairs of one KV head: the work of a sequence depends on its own lengths alone (its output bits do not
 * depend on the batch), and with lq = 1 the output is bit-identical to lvq_attention_decode_ragged on a cache that holds the prefix
 * rows and the own rows one behind the other. */
size_t lvq_attention_extend_shared_workspace_bytes(int batch, int lq, int n_heads, int n_kv_heads, int pmax, int lown, int dh, int precision);
int lvq_attention_extend_shared(const lvq_bf16 *q, const lvq_bf16 *q_lo, const lvq_bf16 *pk_cache, const lvq_bf16 *pk_cache_lo,
                                const lvq_bf16 *pv_cache, const lvq_bf16 *pv_cache_lo, const lvq_bf16 *k_cache, const lvq_bf16 *k_cache_lo,
                                const lvq_bf16 *v_cache, const lvq_bf16 *v_cache_lo, const int32_t *prefix_index, const int32_t *plen,
                                const int32_t *own0, const int32_t *qn, int batch, int lq, int n_heads, int n_kv_heads, int n_prefix,
                                int pmax, int lown, int dh, int64_t q_bstride, int64_t ldq, int64_t q_hstride, int64_t pk_bstride,
                                int64_t k_bstride, int64_t ldk, int64_t k_hstride, int64_t pv_bstride, int64_t v_bstride, int64_t ldv,
                                int64_t v_hstride, int64_t o_bstride, int64_t ldo, int64_t o_hstride, float scale, lvq_bf16 *o,
                                lvq_bf16 *o_lo, void *ws, size_t ws_bytes, lvq_stream_t stream);
/* per-layer prefix caches [n_prefix, pmax, dkv] (post-rotary keys), read-only */
typedef struct {
    const lvq_bf16 *k, *k_lo, *v, *v_lo;
} lvq_qwen2_prefix;
/* The layer loop of lvq_qwen2_decode_step_ragged (inference_engine.py:283-296 -> transformers generate with a KV cache) on batch * lq rows
 * that continue shared prefixes: x [batch, lq, d] fp32 in / out; row r < qn[b] of sequence b is rotated at position
 * plen[prefix_index[b]] + own0[b] + t + r, appended to row own0[b] + t + r of the own caches of `layers` [batch, lown, dkv] and attends
 * as lvq_attention_extend_shared describes; rows r >= qn[b] are padding (nothing appended, output meaningless).  prefix: HOST array of
 * n_layers structs.  own0 is never written: a decode loop passes the question lengths once and t = 0, 1, ... with lq = 1 and qn = 1;
 * the question prefill passes own0 = 0, t = 0.  0 <= t < lown is checked on the host; a row past the own cache
 * (own0[b] + t + r >= lown) is clamped on the device to row lown - 1, which several rows may then write at once: nothing is written
 * outside the cache, but the results of such a sequence are UNDEFINED -- size lown >= max_b(own0[b] + qn[b]) + the tokens to come.  With lq = 1 and batch <= 8 the projections are the calls of lvq_qwen2_decode_step_ragged: output and
 * appended rows are bit-identical to that step on concatenated caches. */
size_t lvq_qwen2_extend_shared_workspace_bytes(int batch, int lq, int d, int n_heads, int n_kv_heads, int inter, int pmax, int lown,
                                               int precision);
int lvq_qwen2_extend_shared(const lvq_qwen2_layer *layers, const lvq_qwen2_prefix *prefix, int n_layers, float *x, int batch, int lq, int d,
                            int n_heads, int n_kv_heads, int inter, const int32_t *prefix_index, const int32_t *plen, int n_prefix, int pmax,
                            const int32_t *own0, const int32_t *qn, int t, int lown, float rms_eps, float rope_theta, int precision, void *ws,
                            size_t ws_bytes, lvq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LVQ_H */
