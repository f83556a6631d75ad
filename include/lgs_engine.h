/*
 * lgs_engine.h -- C-ABI of the MI355X-native sparse-voxel engine (liblgs_engine.so).
 *
 * This is the drop-in boundary UNDER the MinkowskiEngine Python operator surface that
 * RozDavid/LanguageGroundedSemseg is written against.  The reference never binds native code
 * for this path itself -- it calls MinkowskiEngine==0.5.4 (config/lg_semseg.yml:204) through
 * Python -- so every entry point below cites the Python call site(s) of the reference whose
 * work it performs.  The Python host code in languagegroundedsemseg_amd/me/ keeps the ME names
 * (SparseTensor, MinkowskiConvolution, ...) and calls these functions through ctypes.
 *
 * Conventions
 *   - plain C types only; no torch types.  All `const void*` / `void*` buffers are DEVICE
 *     pointers owned by the caller (torch) and only borrowed for the duration of the call.
 *   - compute entry points (conv / bn / ce / clip) enqueue on the HIP stream passed in `stream`
 *     (a hipStream_t cast to void*; NULL = default stream) and never synchronise.
 *   - coordinate-manager entry points build their maps on the manager's OWN stream; `stream` is the
 *     caller's stream, used only for ordering (inputs produced on it are waited for, outputs written
 *     to caller memory are published to it).  lgs_manager_insert and lgs_kmap_export synchronise the
 *     manager's stream once to return a row count to the host (never the caller's compute backlog);
 *     the insert also counts the rows of the eight coarser levels, so lgs_manager_stride2 returns its
 *     count WITHOUT a synchronisation (one host sync per input batch instead of five).  Every compute call that takes an lgs_kmap
 *     orders itself after the manager's map work with a stream-side event wait (no host sync).
 *   - return value: 0 = OK, non-zero = error; lgs_last_error() returns the message of the
 *     last failing call on this thread.  The Python side raises RuntimeError with it.
 *   - a manager and everything it owns is not thread-safe; one manager per input batch
 *     (ME semantics: maps/kernel maps are cached for exactly one forward+backward).
 *   - coords are int32 [N,4] = (batch, x, y, z), batch in column 0
 *     (/root/reference/lib/transforms.py:421, lib/train_test/pl_BaselineTrainer.py:294).
 *     Supported range: batch in [0,1024), |x|,|y|,|z| < 131072 (checked; error otherwise).
 *   - weights are float32 [K, Cin, Cout] (ME parameter layout), kernel-offset index
 *     k enumerates the hypercube with the first spatial axis fastest; odd sizes centred, even
 *     sizes one-sided.  1x1 convs use K = 1.
 *   - features are row-major [N, C] in `dtype` (LGS_F32 or LGS_BF16); accumulation is fp32.
 */
#ifndef LGS_ENGINE_H
#define LGS_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LGS_ABI_VERSION 18

enum lgs_dtype { LGS_F32 = 0, LGS_BF16 = 1 };
enum lgs_supcon_distance { LGS_SUPCON_COS = 0, LGS_SUPCON_L2 = 1 };   /* `distance` of lgs_supcon_forward / lgs_supcon_backward */

typedef struct lgs_manager lgs_manager; /* coordinate manager: owns coordinate maps + kernel maps */
typedef struct lgs_kmap lgs_kmap;       /* one cached kernel map (owned by its manager) */
typedef struct lgs_segmap lgs_segmap;   /* one cached segment map: pooling / broadcast (owned by its manager) */

/* ---- library ---------------------------------------------------------------------------- */
int lgs_abi_version(void);
const char *lgs_last_error(void);

/* ---- tuning table and dispatch counters (csrc/lgs_tuning.hip) -----------------------------
 * No counterpart in the reference (MinkowskiEngine exposes no such hooks): this is the engine's ONE table of tuning and
 * debugging knobs (which used to be scattered getenv calls) and the test hook the parity suite needs to prove coverage.
 *   lgs_tuning_set / get : knob by name ("WW_MIN_ROWS" or "LGS_WW_MIN_ROWS"); initial value = environment LGS_<NAME>, else the
 *                          default.  Unknown name -> error.  Knobs take effect at the next launch.
 *   lgs_tuning_describe  : "NAME\tdefault\tvalue\tdoc\n" per knob into buf (at most cap bytes incl. NUL); returns bytes needed.
 *   lgs_debug_dispatch_counts : "count\tlaunch site\n" for every kernel launch site hit since the last reset (site = kernel
 *                          expression + template bindings, e.g. "k_wgrad_ps<KIND,NCS> [KIND=0,NCS=3]"); reset != 0 zeroes them.
 *                          tests/test_gpu_dispatch_coverage.py: every site the benchmarked steps of bench.py dispatch
 *                          (/root/reference/scripts/train_models.sh, text_representation_train.sh) must also be dispatched
 *                          by a parity test.                                                  */
int lgs_tuning_set(const char *name, int64_t value);
int lgs_tuning_get(const char *name, int64_t *value);
int64_t lgs_tuning_describe(char *buf, int64_t cap);
int64_t lgs_debug_dispatch_counts(char *buf, int64_t cap, int reset);

/* ---- coordinate manager ------------------------------------------------------------------
 * replaces: ME.SparseTensor(features, coordinates) -> CoordinateManager.insert_and_map
 *   /root/reference/lib/train_test/pl_BaselineTrainer.py:300
 *   /root/reference/lib/train_test/pl_RepresentationTrainer.py:183
 *   /root/reference/downstream/insseg/lib/pl_Trainer.py:263                                  */
int lgs_manager_create(int device, lgs_manager **out);
int lgs_manager_destroy(lgs_manager *mgr);
/* Insert coords[N,4] as the tensor-stride-1 map.  Dedups (first occurrence wins, surviving
 * rows keep input order).  Writes the map key to *key and the unique-row count to *n_unique
 * (host; this call synchronises `stream` once).
 * unique_index (device int64[N], first n_unique valid) and inverse (device int64[N]) may be NULL. */
int lgs_manager_insert(lgs_manager *mgr, const int32_t *coords, int64_t n, int64_t *unique_index,
                       int64_t *inverse, void *stream, int *key, int64_t *n_unique);

/* Coarsen map `in_key` by 2 per axis: unique floor(c / 2ts) * 2ts per batch.  Reuses the map if it
 * already exists (ME: one map per tensor stride).  Synchronises `stream` once when it creates one.
 * replaces: the output-coordinate generation inside conv(kernel_size=2, stride=2)
 *   /root/reference/models/res16unet.py:49-56,66-73,83-90,100-107                              */
int lgs_manager_stride2(lgs_manager *mgr, int in_key, void *stream, int *out_key, int64_t *n_out);
/* Device-side consistency flags of this manager's maps, read back with ONE synchronisation of the manager's map stream
 * (test / debug infrastructure: the map builders size coarse maps from counts taken at insert time and never synchronise;
 * a builder that finds its own count disagreeing raises the flag instead of writing past its arrays).  *flags: 0 = consistent,
 * bit 0 = coordinate out of the key range at insert, bit 1 = a coarse map's row count differs from the insert-time count,
 * bit 2 = the origin map's row count differs from the insert-time batch count, bit 3 = a map's lookup table (3^3 neighbour lookup: the block
 * directory, or the hash table of MAP_BLOCK_DIR = 0) was found full while it was filled, which its sizing at twice the entries rules out.
 * Same call sites as lgs_manager_stride2.                                                                             */
int lgs_manager_check(lgs_manager *mgr, int *flags);

/* Finer map that `key` was coarsened from (-1 if none); used by transposed convs to land on the
 * cached map (/root/reference/models/res16unet.py:116-124 + me.cat at :237). */
int lgs_manager_parent_of(lgs_manager *mgr, int key, int *fine_key);

int lgs_manager_map_size(lgs_manager *mgr, int key, int64_t *n, int *tensor_stride);
/* coords of map `key` into dst (device int32 [n,4]); replaces SparseTensor.C (pl_BaselineTrainer.py:384) */
int lgs_manager_get_coords(lgs_manager *mgr, int key, int32_t *dst, void *stream);

/* Nearest site of map `key` for every one of m points: rows[i] = the ROW of the map (at any tensor stride ts) whose site is nearest
 * to point i, -1 where there is none.  A NEW SYMBOL ONLY: LGS_ABI_VERSION stays 18.
 * The site frame: the sites are the integer lattice points c / ts.  Point q of scene s becomes p = (A_s (q, 1)) / ts - anchor, A_s the
 * scene's 3x4 row-major affine evaluated in double as lgs_voxelize does (affines: HOST double [b, 12], read during the call; NULL =
 * the identity).  anchor = 0.0 measures to the voxel corners coords * voxel_size (test_pointcloud's KD-tree), 0.5 to the voxel
 * centres coords + 0.5 (get_original_pointcloud).  With h = rint(p) and f = p - h rounded to fp32 once, the distance to the site at
 * integer offset k from h is d2 = ((f.x - k.x)^2 + (f.y - k.y)^2) + (f.z - k.z)^2 in fp32, each step rounded, in this order; the
 * smallest (d2, row) wins, so among equal d2 the smallest row index.  d2 (device float [m], or NULL) receives it, in site-frame
 * units squared.  Nearest in the site frame is nearest in world space only where A_s is a similarity.
 * scene_offsets: DEVICE int64 [b + 1] as in lgs_voxelize_batched, 1 <= b <= LGS_AUG_MAX_SCENES; points of scene s are matched only
 * against sites with batch index batch_base + s.  A non-finite point, and a point of a scene without sites, gets row -1 and
 * d2 = +inf; a map without rows gives that to every point; m == 0 launches nothing.
 * How: a ring search through the map's lookup table (block directory or hash, MAP_BLOCK_DIR) up to ring NEAREST_MAX_RING, then an
 * exact scan of the scene's sorted keys for what is left -- same arithmetic, same answer at every knob value.  No host
 * synchronisation: the work runs on the map stream, after the caller's pending work and before its later work.
 * Null arguments, unknown keys and the origin map are refused.
 * replaces: spatial.KDTree(pred[:, :3]).query(query_xyz)          /root/reference/lib/datasets/scannet.py:420-421
 *           the pykeops argKmin of get_original_pointcloud         /root/reference/downstream/insseg/datasets/scannet.py:161-169 */
int lgs_manager_nearest(lgs_manager *mgr, int key, const float *points, int64_t m, const int64_t *scene_offsets, int b,
                        int batch_base, const double *affines, double anchor, int64_t *rows, float *d2, void *stream);

/* Kernel map between two maps of this manager (cached per (in_key,out_key,kernel_size)).
 *   kernel_size 3, in_key == out_key            : 3x3x3 stride-1 (a4)
 *   kernel_size 2, out_key == stride2(in_key)   : 2x2x2 stride-2 (a5); the transposed conv (a6)
 *                                                 uses the same object with `transposed` views
 *   kernel_size 1, in_key == out_key            : identity (a7)
 * Everything else is refused here, as it always was; the strided 3^3 / 1x1 and the dilated 3^3 relations are
 * lgs_manager_kernel_map_ex's (below).
 * replaces: the implicit kernel-map construction in MinkowskiConvolution[Transpose].forward
 *   /root/reference/models/modules/common.py:179-236                                           */
int lgs_manager_kernel_map(lgs_manager *mgr, int in_key, int out_key, int kernel_size, void *stream,
                           lgs_kmap **out);

/* The kernel maps of the ResNet encoder family (models/resnet.py: conv(kernel_size=3, stride=2), conv(kernel_size=1, stride=2),
 * dilation= on every 3x3x3 conv of a block).  A NEW SYMBOL ONLY: LGS_ABI_VERSION stays 18, no existing entry point or struct
 * changes; a library that lacks the symbol lacks the capability.  Cached per (in_key, out_key, kernel_size, dilation).
 * With dilation == 1 and one of the three relations above it returns the very object lgs_manager_kernel_map returns.  New:
 *   kernel_size 3, in_key == out_key, dilation d >= 2 : 3x3x3 stride-1 with offsets (-1,0,1) * d * tensor_stride, K = 27, centred,
 *                                                       first spatial axis fastest
 *   kernel_size 3, out_key == stride2(in_key), d == 1 : 3x3x3 stride-2: c_in = c_out + off_k * tensor_stride(in), K = 27; the output
 *                                                       rows are the stride-2 map's
 *   kernel_size 1, out_key == stride2(in_key), d == 1 : 1x1 stride-2: the fine row at the coarse row's coordinate, if any, K = 1
 * Stride 2 combined with dilation > 1 is refused, and so is every other combination.  Offsets that leave the coordinate range
 * have no pair; dilation * tensor_stride must stay below 2^17.  Every conv entry point below takes the new maps with
 * `transposed` 0 and 1.                                                                                             */
int lgs_manager_kernel_map_ex(lgs_manager *mgr, int in_key, int out_key, int kernel_size, int dilation, void *stream,
                              lgs_kmap **out);

/* lgs_debug_kmap_relation: what the two entry points above decide for a request, given by plain facts instead of a live manager, and
 * what follows from the answer for every consumer of the map.  It is the classifier and the table the entry points, the plans and
 * the conv entry points themselves read (csrc/lgs_common.h: classify_kmap, traits_of), so it runs without a GPU
 * (tests/test_kmap_relation_cpu.py holds it to the contract above).  A new symbol only: LGS_ABI_VERSION stays 18.
 * Returns what the entry point would return for the request: 0, or 2 with the refusal in lgs_last_error(). */
typedef struct lgs_kmap_relation_query {
  int entry;                  /* 0 lgs_manager_kernel_map (no dilation argument: the field is ignored), 1 lgs_manager_kernel_map_ex */
  int ks, dilation;
  int link;                   /* 0 in_key == out_key, 1 out_key == stride2(in_key), 2 in_key == stride2(out_key), 3 unrelated keys */
  int tensor_stride;          /* of the in map */
  int out_sorted;             /* the out map's rows are in Morton order (every map made by lgs_manager_stride2) */
  int in_origin, out_origin;  /* the map is lgs_manager_origin's */
} lgs_kmap_relation_query;
typedef struct lgs_kmap_relation_info {
  int rc;                     /* the return value, again */
  int relation;               /* 0 identity 1x1, 1 3^3 stride 1, 2 2^3 stride 2, 3 3^3 dilated stride 1, 4 3^3 stride 2, 5 1x1 stride 2;
                                 -1 refused (the fields below are then 0) */
  int K;                      /* weight matrices */
  int strided;                /* the out map is the in map's stride-2 map */
  int bwd_mirror;             /* the dgrad side is the forward table read mirrored (weight index K-1-s) */
  int transposed_ok;          /* the conv entry points take `transposed` = 1 on the map */
  int pairs_only[2];          /* [transposed]: the weight gradient goes to the pair-list / fp32 kernels only */
  int served_by_old_entry;    /* lgs_manager_kernel_map builds it too (the same object) */
} lgs_kmap_relation_info;
int lgs_debug_kmap_relation(const lgs_kmap_relation_query *q, lgs_kmap_relation_info *out);

/* Export the map as (k, in_row, out_row) triples for set-equality parity tests.
 * Pass NULL buffers to query *m only (synchronises). Buffers are device int32[*m]. */
int lgs_kmap_export(lgs_kmap *km, int32_t *k, int32_t *in_row, int32_t *out_row, void *stream, int64_t *m);

/* lgs_debug_kmap_tables: read-only copy of one view's gather tables exactly as the conv kernels read them (bwd = 0: the forward view,
 * 1: the dgrad view), for tests that compare two ways of building the same map element by element (the tuning knobs MAP_WINDOW_SORT
 * and MAP_BLOCK_DIR).  Always answers *n_pad (positions of the view), *slots (27 / 8 / 1) and *present (bit 0 nbr, bit 1 out_row,
 * bit 2 mask64: which tables the view has).  Non-NULL device buffers nbr int32[slots * n_pad], out_row int32[n_pad] and
 * mask64 uint32[n_pad / 64] receive the tables that are present, ordered on `stream`.  No counterpart in the reference.              */
int lgs_debug_kmap_tables(lgs_kmap *km, int bwd, int32_t *nbr, int32_t *out_row, uint32_t *mask64, void *stream, int64_t *n_pad,
                          int *slots, int *present);

/* ---- pooling, global pooling and broadcast (ABI 14; csrc/lgs_pool.hip) ----------------------
 * replaces MinkowskiSumPooling / AvgPooling / MaxPooling / PoolingTranspose / AvgUnpooling (kernel_size == stride == 2^k),
 * MinkowskiGlobal{Sum,Avg,Max}Pooling and MinkowskiBroadcast{,Addition,Multiplication,Concatenation}:
 *   /root/reference/models/modules/common.py:239-300, models/resnet.py:48, models/resunet.py:367,388,409,
 *   downstream/insseg/lib/layers.py
 * lgs_manager_origin: the origin map of the manager -- one row (b, 0, 0, 0) per batch index of the insert, ascending, tensor
 *   stride 0.  Its row count was taken at insert time: no synchronisation.  Cached.
 * lgs_manager_segment_map: the fine -> coarse relation between `fine_key` and `coarse_key`, where the coarse map is the origin
 *   map or a stride-2^k descendant of the fine map (lgs_manager_stride2 applied k times, 1 <= k <= 12).  Each coarse row owns
 *   one contiguous run of the fine map's Morton-sorted positions.  Built on the manager's stream, cached per key pair; the
 *   compute calls below order themselves after it.
 * lgs_seg_reduce: out[q] = reduction over the fine rows of coarse row q of x (row stride x_ld elements; out [n_coarse, c]
 *   contiguous).  op 0 sum, 1 average (sum / rows present), 2 max (argmax[q][c] = the fine row that won, the smallest row on
 *   ties; int32 [n_coarse, c]), 3 sum of x * x2 (x2 with the same row stride).  fp32 accumulation in a fixed order, one
 *   rounding to `dtype`, no atomics.  `workspace`: lgs_seg_workspace_bytes(sm, c) bytes (0 for maps of stride 2, 4 and 8).
 * lgs_seg_broadcast: for every fine row r of coarse row q: out[r] (row stride out_ld) = op 0 g[q], 1 g[q] / rows of q,
 *   2 x[r] + g[q], 3 x[r] * g[q], 4 x[r] (g unused; the other half of a concatenation).  g is [n_coarse, c] contiguous.
 * lgs_seg_max_backward: dx[r][c] = (argmax[q][c] == r) ? dy[q][c] : 0 for every fine row r (dx, dy contiguous).
 * lgs_segmap_size: rows of the fine and the coarse map. */
int lgs_manager_origin(lgs_manager *mgr, void *stream, int *out_key, int64_t *n_out);
int lgs_manager_segment_map(lgs_manager *mgr, int fine_key, int coarse_key, void *stream, lgs_segmap **out);
int lgs_segmap_size(const lgs_segmap *sm, int64_t *n_fine, int64_t *n_coarse);
int64_t lgs_seg_workspace_bytes(const lgs_segmap *sm, int c);
int lgs_seg_reduce(lgs_segmap *sm, int op, const void *x, const void *x2, int64_t x_ld, int c, void *out, int32_t *argmax,
                   int dtype, void *workspace, void *stream);
int lgs_seg_broadcast(lgs_segmap *sm, int op, const void *g, int c, const void *x, int64_t x_ld, void *out, int64_t out_ld,
                      int dtype, void *stream);
int lgs_seg_max_backward(lgs_segmap *sm, const void *dy, const int32_t *argmax, int c, void *dx, int dtype, void *stream);

/* ---- instance normalisation (ABI 18; csrc/lgs_instnorm.hip) --------------------------------
 * replaces MinkowskiInstanceNorm forward + autograd backward:
 *   /root/reference/models/clip_models.py:408-437, models/modules/resnet_block.py:64-70,126-132, models/modules/common.py:17-27
 *   mean / biased variance per (scene, channel), y = (x - mean) / sqrt(var + eps) * weight + bias; a scene = one batch index.
 * `sm` is lgs_manager_segment_map(mgr, key of x, lgs_manager_origin's key): any other segment map is refused.  x, y, dy, dx are
 * [n_fine, c] contiguous in the rows of x's map; weight, bias, dweight, dbias fp32 [c]; stats fp32 [n_seg][2c] = mean, rstd per
 * scene (written by the forward, read by the backward; y is not kept).  Statistics are summed about the scene's first row in
 * fp32 runs folded in double in a fixed order: no atomics, the same bits on every run.  n_fine == 0: no launch, success (the
 * backward zeroes dweight / dbias).  workspace: lgs_in_workspace_bytes(sm, c) bytes, one size for both directions and dtypes. */
int64_t lgs_in_workspace_bytes(const lgs_segmap *sm, int c);
int lgs_in_forward(lgs_segmap *sm, const void *x, int c, const float *weight, const float *bias, float eps, void *y,
                   float *stats /* [n_seg][2c] mean, rstd */, int dtype, void *workspace, void *stream);
int lgs_in_backward(lgs_segmap *sm, const void *x, const void *dy, int c, const float *weight, const float *stats, void *dx,
                    float *dweight, float *dbias, int dtype, void *workspace, void *stream);

/* ---- sparse convolution --------------------------------------------------------------------
 * replaces MinkowskiConvolution / MinkowskiConvolutionTranspose forward + autograd backward
 *   /root/reference/models/modules/common.py:195-203 (conv), :228-236 (conv_tr)
 *   call sites /root/reference/models/res16unet.py:196-270, models/modules/resnet_block.py:41-57
 *
 * `transposed` = 0: forward direction of the map (in rows -> out rows);
 *                1: the transposed convolution (map's out rows -> map's in rows).
 * `weight` is always the module's own parameter [K,Cin,Cout] (float32), Cin/Cout being THIS
 * op's input/output channels.  `workspace` must hold lgs_conv_workspace_bytes(...) bytes.
 * Zero-copy ME.cat (/root/reference/models/res16unet.py:237,247,257,267): both inputs of a concat are written straight
 * into the concat buffer (lgs_bn_forward's y_row_stride), so the SKIP half is afterwards a column slice of a wider
 * row-major tensor; its readers take a row stride: lgs_conv_forward / lgs_conv_wgrad `in_row_stride` (the strided conv that
 * consumes the skip tensor; bf16 only for wgrad) and lgs_bn_backward `y_row_stride` (the ReLU mask of the norm that
 * produced it).  Rows must stay 16-byte aligned. */
int64_t lgs_conv_workspace_bytes(const lgs_kmap *km, int cin, int cout, int dtype, int op /*0 fwd,1 dgrad,2 wgrad*/);

/* Packed weight images.  The conv kernels read the weights in MFMA fragment order (bf16 / fp32, padded to the tile
 * configuration of the launch shape); by default every call re-packs the fp32 [K,Cin,Cout] parameter into its workspace
 * (~6 us, 125 launches per Res16UNet34C step).  A caller that keeps the image across calls asks lgs_conv_pack_desc for
 * its layout (bytes == 0: this shape packs internally only), owns a device buffer of `bytes`, and passes it as `packed`:
 *   pack_mode 1 = pack into it now, then run;  2 = it is up to date, run straight away;  (packed == NULL: mode 0, internal).
 * lgs_pack_weights_batch re-packs ANY number of images in one launch (descs_device = device copy of the descriptors
 * with `weight` / `packed` filled in, max_total = largest `total`): the host wrapper runs it once after the optimiser
 * step, so the convolutions of the next step find their images ready. */
typedef struct lgs_pack_desc {
  const float *weight; /* device float32 [K, cin_w, cout_w] */
  void *packed;        /* device buffer of `bytes` */
  int64_t bytes, total;
  int K, cin_w, cout_w, transposed, mirror, g_real, o_real, ncp, nbp, dtype;
} lgs_pack_desc;
int lgs_conv_pack_desc(const lgs_kmap *km, int op /* 0 forward, 1 dgrad */, int transposed, int cin, int cout, int dtype,
                       lgs_pack_desc *out);
int lgs_pack_weights_batch(const lgs_pack_desc *descs_device, int n, int64_t max_total, void *stream);

/* out[n_out,cout] = conv(in[n_in,cin]) (+ bias[cout] if non-NULL)
 * bn_partial (may be NULL): the BatchNorm that follows the conv in every block of the model family
 *   (/root/reference/models/modules/resnet_block.py:41-57: conv -> norm) needs sum / sum of squares of this output per
 *   channel; the conv epilogue can emit them per position tile -- float32 [rows][2][cout], rows =
 *   lgs_conv_bn_partial_rows(...) (0 = this launch shape cannot, pass NULL) -- as sum(y - pivot), sum((y - pivot)^2) of the
 *   STORED values, so lgs_bn_forward / lgs_bn_stats need not read the output again for their statistics pass.
 *   bn_pivot: float32 [cout] per-channel shift (BatchNorm's running mean), NULL = 0. */
int lgs_conv_bn_partial_rows(const lgs_kmap *km, int transposed, int cout, int dtype);
int lgs_conv_forward(lgs_kmap *km, int transposed, const void *in, int cin, const float *weight, int cout,
                     const float *bias, void *out, int dtype, void *workspace, float *bn_partial, const float *bn_pivot,
                     void *packed, int pack_mode, int in_row_stride /* elements; 0 = cin */, void *stream);
/* grad_in[n_in,cin] from grad_out[n_out,cout] */
int lgs_conv_dgrad(lgs_kmap *km, int transposed, const void *grad_out, int cout, const float *weight, int cin,
                   void *grad_in, int dtype, void *workspace, void *packed, int pack_mode, void *stream);

/* grad_in += dgrad(grad_out): the sum autograd forms when the convolution's input also feeds a residual branch
 * (models/modules/resnet_block.py:41-57: `out += residual`), taken in the kernel epilogue and rounded exactly like "store the
 * dgrad, then add the two tensors".  lgs_conv_dgrad_can_accumulate() tells whether the launch shape of (km, transposed, cin,
 * cout, dtype) has that epilogue (1) or the caller has to add the tensors itself (0); lgs_conv_dgrad_accumulate() fails
 * for a shape that has not. */
int lgs_conv_dgrad_can_accumulate(const lgs_kmap *km, int transposed, int cin, int cout, int dtype);
int lgs_conv_dgrad_accumulate(lgs_kmap *km, int transposed, const void *grad_out, int cout, const float *weight, int cin,
                              void *grad_in, int dtype, void *workspace, void *packed, int pack_mode, void *stream);
/* grad_weight[K,cin,cout] (float32, overwritten) */
int lgs_conv_wgrad(lgs_kmap *km, int transposed, const void *in, int cin, const void *grad_out, int cout,
                   float *grad_weight, int dtype, void *workspace, int in_row_stride /* elements; 0 = cin */, void *stream);
/* 1 if the kernel that serves this call reads `in` through a row stride in place (k_wgrad_ps without padded rows and
 * k_wgrad_wide do; neither serves e.g. >= 4 GiB at the wider stride or odd channel counts), else 0: the caller then passes a
 * contiguous copy.  The Python host asks before every strided weight gradient instead of letting the call fail. */
int lgs_conv_wgrad_supports_stride(const lgs_kmap *km, int transposed, int cin, int cout, int dtype, int in_row_stride);

/* lgs_debug_conv_plan: the launch plan of a forward (op 0) / dgrad (op 1) convolution on a SYNTHETIC kernel map given by plain
 * integers, plus what the four public queries answer for that map.  No HIP call and no table is read, so it runs without a GPU
 * (tests/test_conv_plan_cpu.py holds the plan to a recorded table and checks that the workspace regions are sound).        */
typedef struct lgs_conv_plan_view {
  int64_t n_pad, n_in, n_out;
  int KS, K;                                /* slots per position, weight matrices */
  int has_nbr, has_tile_k, has_out_row;     /* which tables the view carries (a view with nbr and KS > 1 also has mask64) */
} lgs_conv_plan_view;
typedef struct lgs_conv_plan_query {
  lgs_conv_plan_view fwd, bwd;
  int ks;                                   /* kernel size of the map: 1 / 2 / 3 */
  int op, transposed, cin, cout, dtype;
  int epilogue;                             /* 0 none, 1 BatchNorm statistics, 2 accumulate */
} lgs_conv_plan_query;
typedef struct lgs_conv_plan_region { int64_t offset, bytes; } lgs_conv_plan_region;
typedef struct lgs_conv_plan_info {
  int path;                                 /* 0 empty map, 1 k_pointwise, 2 k_pointwise_f32, 3 k_conv_wide, 4 k_conv_gather */
  int tile_id, sc, wb, tm;                  /* tile configuration of the packed image (whichever path runs) */
  int nc, nb_total, ncp, nbp, gc, wld;
  int64_t total;                            /* uint4 of the packed image */
  int pad_input, scratch_out, packed_ext_ok, split, bn_rows, can_accumulate;
  int64_t grid_x; int grid_y, grid_z;       /* k_conv_gather launches only, else 0 */
  lgs_conv_plan_region packed, padded_in, scratch, bias, partials;
  int64_t bytes_total;
  /* the public queries on the same map */
  int64_t workspace_bytes;
  int q_bn_partial_rows, q_can_accumulate;
  lgs_pack_desc pack_desc;
} lgs_conv_plan_info;
int lgs_debug_conv_plan(const lgs_conv_plan_query *q, lgs_conv_plan_info *out);
/* lgs_debug_conv_gather_residency: how many workgroups of a bf16 k_conv_gather instance the GPU holds per CU
 * (hipOccupancyMaxActiveBlocksPerMultiprocessor; needs a GPU).  Any instance a launch can run: a tile id with scl = chunks per
 * walked slab (the tile's own slab length or 0: its own instance; e.g. tile_id 7 with 1 / 2 / 3, tile_id 2 with 3 / 4);
 * bn_stats = 1: the instance with the BatchNorm statistics epilogue (what a launch with statistics, and every launch
 * under CONV_LEAN_EPI=0, runs), 0: the one without.  A NEW SYMBOL ONLY: LGS_ABI_VERSION stays 18. */
int lgs_debug_conv_gather_residency(int tile_id, int scl, int bn_stats, int *workgroups_per_cu);
/* lgs_debug_conv_gather_instance: which instance of k_conv_gather the launch of that plan runs (the query must plan path 4), with
 * BatchNorm statistics (forward launches whose plan has statistic rows) or without.  No HIP call, like lgs_debug_conv_plan
 * (tests/test_conv_instance_cpu.py holds it to a recorded table).  A NEW SYMBOL ONLY: LGS_ABI_VERSION stays 18. */
typedef struct lgs_conv_gather_instance {
  int tile_id;                              /* the plan's */
  int scl, row1;                            /* chunks per walked slab, 0 = the tile's own instance; the one-piece-row walk */
  int bn, onebuf;                           /* with the statistics epilogue; one weight slab in LDS */
  int rb, ncb, wm, wn, sc, d;               /* the instance's <RB, NCB, WM, WN, SC, D> for the dtype */
  char site[160];                           /* the launch site the launch is counted at (lgs_debug_dispatch_counts) */
} lgs_conv_gather_instance;
int lgs_debug_conv_gather_instance(const lgs_conv_plan_query *q, int with_statistics, lgs_conv_gather_instance *out);

/* lgs_debug_wgrad_plan (ABI 16): the same for lgs_conv_wgrad -- which kernel serves the call, its launch parameters and workspace
 * regions, and what lgs_conv_workspace_bytes(op 2) / lgs_conv_wgrad_supports_stride answer on that map
 * (tests/test_wgrad_plan_cpu.py).  One partial slab is [K][pad_a][pad_b] floats, whichever kernel writes it. */
typedef struct lgs_wgrad_plan_query {
  lgs_conv_plan_view fwd, bwd;
  int ks, transposed, cin, cout, dtype, in_row_stride;
} lgs_wgrad_plan_query;
typedef struct lgs_wgrad_plan_info {
  int path;                /* 0 empty map, 1 k_wgrad_wide, 2 k_wgrad_ps, 3 k_wgrad_bf16 (pair list), 4 fp32 (k_wgrad_f32*) */
  int bwd_view;            /* the view the kernel walks: 0 the map's fwd, 1 its bwd */
  int in_place;            /* 1: the kernel reads `in` through in_row_stride as it lies */
  int pad_in, pad_gout;    /* channels the input / gradient rows are zero-padded to in the workspace, 0 = read as they are */
  int all_cus;             /* k_wgrad_ps: all 32 CUs of every XCD instead of PS_CUS (the padded colour input) */
  int f32_kernel;          /* fp32 path, operands on the 16-byte grid: 0 k_wgrad_f32, 1 k_wgrad_f32_lds, 2 k_wgrad_f32s_lds */
  int t0, t1;              /* template parameters: KIND, NCS (k_wgrad_ps) / NCI, NCO (k_wgrad_bf16) / NCB, 0 (fp32) */
  int pad_a, pad_b;        /* channel extents of a partial slab */
  int slots;               /* partial slabs per kernel offset set: ps lanes / pair-list and fp32 slots / wide position ranges */
  int64_t span;            /* positions per slot, range (pair list, fp32) or workgroup range (wide) */
  int n_ranges, kpw;       /* k_wgrad_bf16: position ranges dealt to the slots, kernel offsets per workgroup */
  int tasks_a, tasks_b;    /* channel tiles per slab side: ci / co tasks, gathered / stationary slices, 256-channel tiles */
  int cpl, n_chunks, xcd_map;   /* k_wgrad_ps: chunks per lane, 128-position chunks, slices of a lane pinned to one XCD */
  int ntile;               /* k_wgrad_wide: 256-position compaction tiles */
  int64_t grid_x; int grid_y, grid_z, lds_bytes;   /* the main launch (dynamic LDS) */
  int64_t reduce_blocks;   /* 256-thread workgroups of the reduce launch */
  lgs_conv_plan_region partials, padded_in, padded_gout, ww_count, ww_offset, ww_total, ww_pair_in, ww_pair_out;
  int64_t bytes_total;
  /* the public queries on the same map */
  int64_t workspace_bytes;
  int supports_stride;
} lgs_wgrad_plan_info;
int lgs_debug_wgrad_plan(const lgs_wgrad_plan_query *q, lgs_wgrad_plan_info *out);

/* ---- fused batch-norm / ReLU / residual ------------------------------------------------------
 * replaces ME.MinkowskiBatchNorm (.bn = nn.BatchNorm1d over all rows) + MinkowskiReLU + `out += residual`
 *   /root/reference/models/modules/common.py:17-19, models/modules/resnet_block.py:41-57
 * Training-mode batch statistics over all n rows.  stats = float32 [2*C] workspace:
 * on return mean[C], invstd[C].  running_mean/var (float32 [C]) updated with `momentum`
 * (unbiased variance), may be NULL; num_batches_tracked (device int64 scalar, nn.BatchNorm1d's buffer) is
 * incremented by the same kernel, may be NULL.  residual may be NULL.  y may alias x.
 * workspace: lgs_bn_workspace_bytes(n, c) bytes of caller-owned device scratch (no allocation inside).  The size is the bound
 * over every path a BatchNorm entry point can take for (n, c) -- it depends on neither dtype, direction nor the tuning table, so
 * a caller may keep it per (n, c) and use one buffer for lgs_bn_forward / backward / stats / backward_reduce, whatever the
 * knobs are when the call is made.
 * conv_partials / conv_partial_rows / pivot: statistics already produced by the preceding lgs_conv_forward (see there);
 * NULL / 0 = compute them from x. */
int64_t lgs_bn_workspace_bytes(int64_t n, int c);
int lgs_bn_forward(const void *x, int64_t n, int c, const float *gamma, const float *beta, float eps,
                   float momentum, float *running_mean, float *running_var, int64_t *num_batches_tracked,
                   const void *residual, int relu, void *y, float *stats, int dtype, void *workspace,
                   const float *conv_partials /* lgs_conv_forward's bn_partial or NULL */, int conv_partial_rows,
                   const float *pivot /* the bn_pivot that conv call was given */, int64_t y_row_stride /* elements; 0 = c */,
                   void *stream);
/* Backward of the fused op.  x = forward input, stats = the forward's mean/invstd.
 * relu: 0 = none; 1 = ReLU mask taken from the forward OUTPUT y (required when a residual was added);
 *       2 = mask recomputed from x as (xhat*gamma + beta > 0), y may be NULL (one tensor read fewer).
 * Writes dx, dgamma[C], dbeta[C]; if dresidual != NULL also the gradient flowing to the residual (= masked dy).
 * dy_row_stride (elements, 0 = C): dy may be a column slice of a wider row-major tensor -- the gradient of one input
 * of ME.cat (res16unet.py:233-262) is exactly that, and reading it in place saves a copy of the whole slice. */
int lgs_bn_backward(const void *x, const void *y, const void *dy, int64_t dy_row_stride, int64_t n, int c,
                    const float *gamma, const float *beta, const float *stats, int relu, void *dx, void *dresidual,
                    float *dgamma, float *dbeta, int dtype, void *workspace, int64_t y_row_stride /* of y; 0 = c */,
                    void *stream);

/* The same op in halves, so that data-parallel training can exchange the statistics between ranks in the middle
 * (ME.MinkowskiSyncBatchNorm, /root/reference/main.py:122-123) with one small collective per direction and NO host-side
 * tensor arithmetic in between:
 *   lgs_bn_stats           -> rec[2C+1] = local mean[C], local M2[C] (sum of squared deviations from it), row count
 *   (all-gather of the records of all ranks: all_stats[world][2C+1])
 *   lgs_bn_sync_combine    -> stats[2C] = global mean, invstd (Chan's parallel formula, double); updates running_mean /
 *                             running_var / num_batches_tracked (each may be NULL); *inv_n_total = 1 / global rows
 *   lgs_bn_apply           <- stats[2C]
 *   lgs_bn_backward_reduce -> sums[2C] = local sum dy', local sum dy' * xhat (dy' = dy masked by ReLU); the same two
 *                             vectors also go to dgamma / dbeta (may be NULL): parameter gradients stay local
 *   (all-reduce of sums)
 *   lgs_bn_backward_apply  <- sums[2C] (all-reduced), 1/N either by value (inv_n_total) or, if inv_n_device != NULL,
 *                             read from the device scalar lgs_bn_sync_combine wrote (no host sync)
 * y_row_stride / dy_row_stride (elements, 0 = c): y / dy may be column slices of wider row-major buffers (zero-copy ME.cat: the
 * norm writes into, and its backward reads from, the concat buffer), rows 16-byte aligned. */
int lgs_bn_stats(const void *x, int64_t n, int c, float *rec /* [2C+1] */, int dtype, void *workspace,
                 const float *conv_partials, int conv_partial_rows, const float *pivot, void *stream);
int lgs_bn_sync_combine(const float *all_stats, int world, int c, float eps, float momentum, float *running_mean,
                        float *running_var, int64_t *num_batches_tracked, float *stats, float *inv_n_total, void *stream);
int lgs_bn_apply(const void *x, int64_t n, int c, const float *gamma, const float *beta, const float *stats,
                 const void *residual, int relu, void *y, int dtype, int64_t y_row_stride, void *stream);
int lgs_bn_backward_reduce(const void *x, const void *y, const void *dy, int64_t n, int c, const float *gamma,
                           const float *beta, const float *stats, int relu, float *sums, float *dgamma, float *dbeta,
                           int dtype, void *workspace, int64_t dy_row_stride, int64_t y_row_stride, void *stream);
int lgs_bn_backward_apply(const void *x, const void *y, const void *dy, int64_t n, int c, const float *gamma,
                          const float *beta, const float *stats, const float *sums, float inv_n_total,
                          const float *inv_n_device, int relu, void *dx, void *dresidual, int dtype, int64_t dy_row_stride,
                          int64_t y_row_stride, void *stream);

/* lgs_debug_norm_plan (ABI 17): what a BatchNorm call decides on the host, for a call given by plain integers: the path, every
 * grid and rows-per-workgroup, and the workspace regions, plus what lgs_bn_workspace_bytes answers.  resident_cap stands for the
 * one thing the engine asks the device (workgroups of the direction's grid-barrier kernel it holds at once).  No HIP call: it
 * runs without a GPU (tests/test_norm_plan_cpu.py). */
typedef struct lgs_norm_plan_query {
  int direction;           /* 0 lgs_bn_forward, 1 lgs_bn_backward, 2 lgs_bn_stats, 3 lgs_bn_backward_reduce */
  int c, dtype;
  int conv_partial_rows;   /* rows of the conv epilogue's partial sums (directions 0 and 2), 0 = statistics from x */
  int resident_cap;
  int64_t n;
} lgs_norm_plan_query;
typedef struct lgs_norm_plan_info {
  int path;                /* 1 fold (two launches), 2 fused (one grid-barrier launch), 3 three launches */
  int from_partials;       /* 1: the statistics come from the conv epilogue's rows, x is not reduced */
  int reduce_grid;         /* workgroups that reduce x: k_colreduce, or the whole fused launch; 0 = none (path 3 from partials) */
  int64_t rows_per_block;  /* rows of x per workgroup of it */
  int partial_rpb;         /* conv partial rows folded into one row (k_partial_reduce / step 1 of k_bn_fwd_fused), 0 = none */
  int fold_rows;           /* partial rows [2c] the fold reads = rows written to the workspace */
  int fold_grid;           /* path 3: workgroups of k_fold_fwd / k_fold_stats / k_fold_bwd */
  int apply_grid;          /* workgroups of the apply launch of paths 1 and 3; 0 = none (empty tensor, directions 2 and 3) */
  lgs_conv_plan_region partials, sums, spill;   /* partial rows; [2c] sums of lgs_bn_backward; dgamma / dbeta of lgs_bn_backward_reduce */
  int64_t bytes_total;
  int64_t workspace_bytes; /* lgs_bn_workspace_bytes(n, c) */
} lgs_norm_plan_info;
int lgs_debug_norm_plan(const lgs_norm_plan_query *q, lgs_norm_plan_info *out);

/* ---- two norms on the same rows: the residual block's norm2 and its downsample-branch norm (csrc/lgs_norm.hip) ----
 *   /root/reference/models/modules/resnet_block.py:41-57, models/resnet.py:93-103   (out = relu?(norm2(conv2) + norm_d(conv_d(x))))
 * norm a = the main norm (adds the branch, optional ReLU), norm b = the branch norm (no ReLU); both [n, c] of one dtype.
 *   lgs_bn_forward_pair : y = relu?(bn_a(xa) + bn_b(xb)); both norms' saved statistics, running statistics and num_batches_tracked
 *                         exactly as two lgs_bn_forward calls leave them.  res (may be NULL): the branch output bn_b(xb), written
 *                         only when asked for -- the sum uses its value as stored in `dtype`, so y is bit-identical to the two calls.
 *   lgs_bn_backward_pair: both norms receive dy' = dy masked by norm a's ReLU (relu 0 = none, 1 = the mask from ya); writes
 *                         dxa, dxb, both dgamma / dbeta, and dy' to dresidual when it is not NULL.
 * Each direction reads every operand once: one statistics launch for both norms, one fold launch, one apply (`three`: 3 launches;
 * `fold`: 2) instead of the 6 (4) of the single calls, 5 instead of 7 tensor passes forward and 10 instead of 13 backward, same
 * per-element expressions and summation orders (bit-identical results).  The path is the single-norm plan's (lgs_debug_norm_plan)
 * for (direction, n, c, dtype); where that is the grid-barrier `fused` path, where the tuning knob BN_PAIR is 0, and for n == 0 the
 * entry points issue the two single calls (path 0) -- which need their intermediate: res / dresidual must then be given.
 * lgs_bn_pair_plan answers which it is for a call on the current device (it asks the device what lgs_bn_forward / backward ask, and
 * launches nothing); lgs_debug_norm_pair_plan is the same for a resident-workgroup bound given by the caller (no HIP call: it runs
 * without a GPU, tests/test_norm_pair_plan_cpu.py).
 * workspace: lgs_bn_pair_workspace_bytes(n, c) (the bound over every path and knob setting, as lgs_bn_workspace_bytes is).
 * NEW SYMBOLS ONLY: LGS_ABI_VERSION stays 18; a library that lacks them lacks the capability. */
struct lgs_bn_params;
typedef struct lgs_norm_pair_plan_info {
  int path;                /* 0 the two single calls; 1 fold pair (two launches); 3 three-launch pair */
  int single_path;         /* lgs_norm_plan_info.path of the single-norm plan it was derived from */
  int launches;            /* launches of this direction (path 0: of both single calls) */
  int reduce_grid;         /* workgroups (x) of the statistics launch; forward: y = 2, one slice per norm */
  int64_t rows_per_block;
  int fold_rows, fold_grid, apply_grid;   /* as in lgs_norm_plan_info; the fold launch has y = 2 */
  lgs_conv_plan_region partials_a, partials_b, sums_a, sums_b;   /* both norms' partial rows, then (backward, path 3) their [2c] sums */
  int64_t bytes_total;
  int64_t workspace_bytes; /* lgs_bn_pair_workspace_bytes(n, c) */
} lgs_norm_pair_plan_info;
int64_t lgs_bn_pair_workspace_bytes(int64_t n, int c);
int lgs_bn_pair_plan(int direction /* 0 forward, 1 backward */, int64_t n, int c, int dtype, lgs_norm_pair_plan_info *out);
int lgs_debug_norm_pair_plan(const lgs_norm_plan_query *q /* direction 0 or 1; conv_partial_rows ignored */, lgs_norm_pair_plan_info *out);
int lgs_bn_forward_pair(const void *xa, const struct lgs_bn_params *norm_a, float *stats_a, const void *xb,
                        const struct lgs_bn_params *norm_b, float *stats_b, int64_t n, int c, int relu, void *y,
                        int64_t y_row_stride /* elements; 0 = c */, void *res /* may be NULL */, int dtype, void *workspace, void *stream);
int lgs_bn_backward_pair(const void *xa, const void *ya, const float *gamma_a, const float *beta_a, const float *stats_a, int relu,
                         const void *xb, const float *gamma_b, const float *stats_b, const void *dy, int64_t dy_row_stride,
                         int64_t n, int c, void *dxa, void *dxb, float *dgamma_a, float *dbeta_a, float *dgamma_b, float *dbeta_b,
                         void *dresidual /* may be NULL */, int dtype, void *workspace, int64_t ya_row_stride /* of ya; 0 = c */,
                         void *stream);

/* lgs_debug_instnorm_plan (ABI 18): what an instance-norm call decides on the host, for a call given by plain integers (the sizes
 * of the origin segment map: fine rows, scenes, chunk items).  No HIP call: it runs without a GPU (tests/test_instnorm_cpu.py). */
typedef struct lgs_instnorm_plan_query {
  int direction;           /* 0 lgs_in_forward, 1 lgs_in_backward */
  int c, dtype;
  int64_t n_fine, n_seg, n_items;
} lgs_instnorm_plan_query;
typedef struct lgs_instnorm_plan_info {
  int vec;                 /* 1: 16 bytes per lane (c * element size a multiple of 16), 0: one element per lane */
  int lanes_log2;          /* log2 of the lanes that share one row */
  int rows_per_apply_block;
  int64_t reduce_grid;     /* workgroups of k_in_reduce: one per chunk item */
  int64_t combine_grid;    /* workgroups of k_in_combine: scenes x channel blocks */
  int64_t apply_grid;      /* workgroups of k_in_apply; all three are 0 for an empty tensor (no launch) */
  lgs_conv_plan_region partials, sums;   /* item partial rows [n_items][2c]; the backward's per-scene sums [n_seg][2c] */
  int64_t bytes_total;
  int64_t workspace_bytes; /* lgs_in_workspace_bytes(sm, c) */
} lgs_instnorm_plan_info;
int lgs_debug_instnorm_plan(const lgs_instnorm_plan_query *q, lgs_instnorm_plan_info *out);

/* lgs_debug_seg_plan: what a pooling / broadcast call decides on the host, for a call given by plain integers (the sizes of the
 * segment map, whether its segments fit one chunk, and whether the call's operands allow 16-byte accesses).  No HIP call: it
 * runs without a GPU (tests/test_seg_plan_cpu.py). */
typedef struct lgs_seg_plan_query {
  int family;              /* 0 lgs_seg_reduce, 1 lgs_seg_broadcast, 2 lgs_seg_max_backward */
  int c, dtype;
  int single_pass;         /* 1: no segment is longer than one chunk (maps of stride 2, 4 and 8); 0: chunk items + combine */
  int vec_ok;              /* 1: every operand the call dereferences has 16-byte aligned rows (pointer and row stride) */
  int64_t n_fine, n_coarse, n_items;
} lgs_seg_plan_query;
typedef struct lgs_seg_plan_info {
  int vec;                 /* 1: 16 bytes per lane (vec_ok and c * element size a multiple of 16), 0: one element per lane */
  int lanes_log2;          /* log2 of the lanes that share one row in k_seg_reduce / k_seg_bcast / k_seg_max_bwd */
  int combine_lanes_log2;  /* the same for k_seg_combine (one fp32 partial per lane) */
  int64_t reduce_grid;     /* family 0: workgroups of k_seg_reduce over the coarse rows (single pass) or the chunk items */
  int64_t combine_grid;    /* family 0, two passes: workgroups of k_seg_combine; 0 = none */
  int64_t bcast_grid;      /* family 1: workgroups of k_seg_bcast */
  int64_t max_bwd_grid;    /* family 2: workgroups of k_seg_max_bwd; the grids of the other families are 0 */
  lgs_conv_plan_region partials, partial_argmax;   /* family 0, two passes: fp32 [n_items][c] and int32 [n_items][c] */
  int64_t bytes_total;
  int64_t workspace_bytes; /* lgs_seg_workspace_bytes(sm, c) */
} lgs_seg_plan_info;
int lgs_debug_seg_plan(const lgs_seg_plan_query *q, lgs_seg_plan_info *out);

/* ---- SyncBatchNorm as one call per direction, on the engine's own RCCL communicator (csrc/lgs_comm.hip) --------
 * replaces the per-layer statistics exchange of ME.MinkowskiSyncBatchNorm (convert_sync_batchnorm, /root/reference/main.py:121-123;
 * downstream/insseg/lib/ddp_trainer.py:191-194) when it runs rank per GPU: the split kernels above with ncclAllGather /
 * ncclAllReduce issued ON THE CALLER'S STREAM between them (no process-group stream hand-over, no host code in between).
 *   lgs_comm_unique_id   rank 0: 128 opaque bytes (ncclGetUniqueId) for the ranks to share (e.g. one torch.distributed broadcast)
 *   lgs_comm_create      every rank, collectively (ncclCommInitRank on `device`); lgs_comm_destroy releases it
 *   lgs_bn_forward_sync  = lgs_bn_stats -> all-gather [world][2C+1] -> lgs_bn_sync_combine -> lgs_bn_apply; stats [2C] and
 *                          inv_n [1] (device scalar 1 / global rows) are outputs the backward takes back
 *   lgs_bn_backward_sync = lgs_bn_backward_reduce -> all-reduce [2C] -> lgs_bn_backward_apply (dgamma / dbeta stay local)
 * RCCL is resolved at run time from the librccl the process has loaded; without one lgs_comm_* fail with a message and the
 * caller keeps its own collectives.  workspace: lgs_bn_sync_workspace_bytes(n, c, world). */
typedef struct lgs_comm lgs_comm;
int lgs_comm_unique_id(void *id128);
int lgs_comm_create(const void *id128, int world, int rank, int device, lgs_comm **out);
/* Mailbox mode (no RCCL): lgs_comm_create_ipc allocates this rank's mailbox in device memory and returns its 64-byte
 * hipIpcMemHandle; the ranks exchange the handles out of band (one torch.distributed all-gather) and every rank passes ALL of
 * them ([world][64] bytes, its own entry ignored) to lgs_comm_ipc_open.  lgs_bn_forward_sync / lgs_bn_backward_sync then exchange
 * through ONE kernel each (peer-to-peer stores into every rank's mailbox, arrival flags spun on in the kernel) instead of an RCCL
 * collective.  All ranks of one communicator must issue the same sequence of calls.  Same call sites as above. */
int lgs_comm_create_ipc(int world, int rank, int device, lgs_comm **out, void *handle64);
int lgs_comm_ipc_open(lgs_comm *comm, const void *handles64);
int lgs_comm_destroy(lgs_comm *comm);
int lgs_comm_world(const lgs_comm *comm);
int64_t lgs_bn_sync_workspace_bytes(int64_t n, int c, int world);
int lgs_bn_forward_sync(lgs_comm *comm, const void *x, int64_t n, int c, const float *gamma, const float *beta, float eps,
                        float momentum, float *running_mean, float *running_var, int64_t *num_batches_tracked,
                        const void *residual, int relu, void *y, float *stats, float *inv_n, int dtype, void *workspace,
                        int64_t y_row_stride, void *stream);
int lgs_bn_backward_sync(lgs_comm *comm, const void *x, const void *y, const void *dy, int64_t n, int c, const float *gamma,
                         const float *beta, const float *stats, const float *inv_n, int relu, void *dx, void *dresidual,
                         float *dgamma, float *dbeta, int dtype, void *workspace, int64_t dy_row_stride, int64_t y_row_stride,
                         void *stream);

/* ---- one call per residual block and direction (csrc/lgs_block.hip) -----------------------------
 * replaces the call sequence of BasicBlock.forward and of its autograd backward
 *   /root/reference/models/modules/resnet_block.py:41-57   (conv1 - norm1 - relu - conv2 - norm2 - (+ residual) - relu)
 *   /root/reference/models/resnet.py:93-103                 (downsample = 1x1 conv + norm on the residual branch)
 * for batches small enough that the training step is bound by the HOST enqueueing ~250 engine calls (one ~150 k-voxel
 * scene per step).  Exactly the launches of the call-by-call path, in the same order, on the caller's stream: results are
 * bit-identical.  Every pointer is a device pointer owned by the caller; packed weight images / modes as in lgs_conv_forward
 * (forward images for lgs_block_forward, dgrad images for lgs_block_backward).  Training mode only (batch statistics).     */
typedef struct lgs_bn_params {
  const float *gamma, *beta;
  float *running_mean, *running_var;     /* may be NULL together */
  int64_t *num_batches_tracked;          /* may be NULL */
  float eps, momentum;
} lgs_bn_params;
typedef struct lgs_block_fwd {
  lgs_kmap *km3, *km1;                   /* 3^3 map of the level; 1x1 map (NULL = no downsample branch) */
  int dtype, relu_final, cin, planes;
  int64_t n;                             /* rows of the level */
  const void *x;                         /* [n, cin] */
  const float *w1, *w2, *wd;             /* fp32 [27, cin, planes], [27, planes, planes], [cin, planes] or NULL */
  void *pk1, *pk2, *pkd;                 /* packed images (lgs_conv_pack_desc, op 0) or NULL */
  int pm1, pm2, pmd;                     /* pack modes as for lgs_conv_forward */
  lgs_bn_params n1, n2, nd;
  void *o1, *y1, *o2, *od, *res, *y2;    /* [n, planes] outputs: conv1, norm1+relu, conv2, downsample conv, its norm, block output */
  float *st1, *st2, *std_;               /* [2 planes] mean | invstd of the three norms (saved for backward) */
  void *conv_ws, *bn_ws;                 /* lgs_block_workspace_bytes / lgs_bn_workspace_bytes(n, planes); with km1 the branch norm
                                            and norm2 run as lgs_bn_forward_pair / lgs_bn_backward_pair: bn_ws is then
                                            lgs_bn_pair_workspace_bytes(n, planes), and res (forward) / dres (backward) may be NULL
                                            unless lgs_bn_pair_plan answers path 0 for the direction */
} lgs_block_fwd;
typedef struct lgs_block_bwd {
  lgs_kmap *km3, *km1;
  int dtype, relu_final, cin, planes, want_gin, x_row_stride;   /* x_row_stride: elements, 0 = cin (zero-copy cat slices) */
  int64_t n, dy_row_stride;              /* dy_row_stride: elements, 0 = planes */
  const void *dy;                        /* [n, planes] upstream gradient */
  const void *x, *o1, *y1, *o2, *y2, *od;               /* saved by the forward (y2 only when relu_final; od with km1) */
  const float *st1, *st2, *std_;
  const float *w1, *w2, *wd;
  void *pk1, *pk2, *pkd;                 /* packed DGRAD images (lgs_conv_pack_desc, op 1) or NULL */
  int pm1, pm2, pmd;
  const float *gamma1, *beta1, *gamma2, *beta2, *gammad, *betad;
  void *dx2, *dres, *dy1, *dx1, *dxd, *gind;            /* [n, planes] x5 scratch / results, gind [n, cin] (km1 only) */
  float *gw1, *gw2, *gwd;                /* weight gradients, fp32, parameter shapes (e.g. views of gradient-bucket slots) */
  float *dgamma1, *dbeta1, *dgamma2, *dbeta2, *dgammad, *dbetad;
  void *conv_ws, *bn_ws;
  /* weight gradients beside the dgrad / BatchNorm chain (me/modules.py conv_weight_grad does the same call by call): when
   * wgrad_stream is set, every lgs_conv_wgrad of the block is enqueued THERE, ordered after its operands by fork_event
   * (hipEvent_t, re-recorded on `stream` per weight gradient), uses wgrad_ws (its own lgs_conv_workspace_bytes(op 2) scratch)
   * and is followed by a record of ev_w1 / ev_w2 / ev_wd (hipEvent_t, may be NULL) on wgrad_stream -- what the consumer of
   * the gradient (bucketed all-reduce, optimizer) waits for.  NULL: the weight gradients run on `stream`. */
  void *wgrad_stream, *wgrad_ws, *fork_event, *ev_w1, *ev_w2, *ev_wd;
} lgs_block_bwd;                         /* grad_in: dres (no downsample) or gind (with), accumulated in place */
int64_t lgs_block_workspace_bytes(const lgs_kmap *km3, const lgs_kmap *km1, int cin, int planes, int dtype);
int lgs_block_forward(const lgs_block_fwd *args, void *stream);
int lgs_block_backward(const lgs_block_bwd *args, void *stream);

/* ---- CLIP text-anchor contraction (MFMA) ----------------------------------------------------
 * replaces ContrastiveLanguageLoss.feat_dist (cos) + feature_sim
 *   /root/reference/lib/losses/ContrastiveLanguageLoss.py:73-95,185-192
 *   /root/reference/lib/losses/utils.py:80-103
 * S[n, n_anchor] = normalize(F)[n,c] . normalize(T)[n_anchor,c]^T, float32 out.
 * inv_norm_f (float32 [n], may be NULL) receives 1/max(|f|,1e-12) for the backward. */
int lgs_clip_similarity(const void *feat, int64_t n, int c, const float *anchors, int n_anchor, float *sim,
                        float *inv_norm_f, int dtype, void *workspace, void *stream);
int64_t lgs_clip_workspace_bytes(int c, int n_anchor, int dtype);

/* ---- fused CLIP text-anchor loss (forward in ONE pass over the features, 4-sparse backward) --------
 * replaces ContrastiveLanguageLoss.forward's arithmetic (gather [N,1+K,C] + feat_dist bmm) AND feature_sim + argmax
 *   /root/reference/lib/losses/ContrastiveLanguageLoss.py:73-95 (feat_dist, cos), :185-192 (hinge inputs)
 *   /root/reference/lib/losses/utils.py:80-103 (feature_sim, cosine branch) + pl_RepresentationTrainer.py:237-238 (argmax)
 * lgs_clip_loss_forward: per row n (labels[n] == ignore_label, or outside [0, n_anchor): d_pos = d_neg = 0, :94)
 *   d_pos[n] = 1 - <f^_n, t^_labels[n]>,   d_neg[n] = 1 - mean_j <f^_n, t^_neg[n,j]>,   j < k_neg (1..7)
 *   pred[n]  = argmax_a <f^_n, t^_a>  (first maximum; may be NULL),   inv_norm_f[n] = 1 / max(|f_n|, 1e-12)
 *   anchors_n[n_anchor, c] (float32 out) = row-normalised anchors, kept for the backward
 *   sim[n, n_anchor] (float32) is written only when non-NULL (metrics / visualisation): the loss never needs it.
 *   n_anchor % 4 == 0, 4 <= n_anchor <= 224 (a wavefront owns all anchor columns of its rows).
 * lgs_clip_loss_backward: grad_feat[n, c] (dtype) from the upstream g_dpos[n], g_dneg[n] (float32, either may be NULL):
 *   gf = ( sum_j gs_j t^_j - (sum_j gs_j s_j) f^ ) / |f|  with  gs_pos = -g_dpos, gs_neg_j = -g_dneg / k_neg  (zero rows
 *   for ignored labels).  d_pos / d_neg / inv_norm_f / anchors_n are the forward's outputs. */
int64_t lgs_clip_loss_workspace_bytes(int c, int n_anchor, int dtype);
int lgs_clip_loss_forward(const void *feat, int64_t n, int c, const float *anchors, int n_anchor, const int64_t *labels,
                          const int64_t *neg, int k_neg, int64_t ignore_label, float *d_pos, float *d_neg, int64_t *pred,
                          float *inv_norm_f, float *anchors_n, float *sim, int dtype, void *workspace, void *stream);
int lgs_clip_loss_backward(const void *feat, int64_t n, int c, const float *anchors_n, int n_anchor, const int64_t *labels,
                           const int64_t *neg, int k_neg, int64_t ignore_label, const float *inv_norm_f, const float *d_pos,
                           const float *d_neg, const float *g_dpos, const float *g_dneg, void *grad_feat, int dtype,
                           void *stream);
/* lgs_clip_loss_backward_anchors: the same upstream gradient w.r.t. the NORMALISED anchors, for models that learn a projection of
 *   the text anchors (/root/reference/models/clip_models.py:192-200, Res16UNet34CR_Proj):
 *   grad_anchors_t[c][a8] (float32, a8 = n_anchor rounded up to 8; column a = d loss / d t^_a) = F^T G, G the 4-sparse matrix
 *   dL/dS (-g_dpos at the class, -g_dneg / k_neg at each negative, zero rows for ignored labels), as ONE launch of the weight-
 *   gradient kernels over the identity map (fixed summation order).  The caller applies d t^ -> d t (the anchor normalisation). */
int64_t lgs_clip_anchor_grad_workspace_bytes(int64_t n, int c, int n_anchor, int dtype);
int lgs_clip_loss_backward_anchors(const void *feat, int64_t n, int c, int n_anchor, const int64_t *labels, const int64_t *neg,
                                   int k_neg, int64_t ignore_label, const float *inv_norm_f, const float *g_dpos,
                                   const float *g_dneg, float *grad_anchors_t, int dtype, void *workspace, void *stream);

/* ---- fused SGD step on a flat parameter / gradient bucket -----------------------------------------
 * torch.optim.SGD's update rule as the reference configures it (/root/reference/lib/solvers.py: momentum 0.9,
 * dampening 0.1, weight_decay 1e-4) in ONE pass:  d = g + wd*p;  buf = first_step ? d : m*buf + (1-damp)*d;
 * p -= lr * mask * buf.   mask (may be NULL) zeroes the update of parameters that received no gradient this step. */
int lgs_sgd_step(float *params, const float *grads, float *momentum_buf, const float *mask, int64_t n, float lr,
                 float momentum, float dampening, float weight_decay, int first_step, void *stream);

/* ---- voxelisation on the device (the step in front of the hot path) ----------------
 * lgs_voxelize: points[n,3] float32 -> coords[n,4] int32 = (batch, floor(A * (x,y,z,1))), A = 3x4 row-major affine
 *   given as 12 HOST doubles (voxel scale / rotation / translation), evaluated in double like numpy's:
 *   /root/reference/lib/voxelizer.py:136-139 (homo_coords @ rigid_transformation.T[:, :3] -> np.floor) plus the batch
 *   column of ME.utils.sparse_collate (lib/transforms.py:421).
 * lgs_label_vote: label rule of ME.utils.sparse_quantize(..., labels, ignore_label) (lib/voxelizer.py:284): a voxel
 *   keeps its first point's label unless another of its points disagrees -> ignore_label.  unique_index / inverse are
 *   the outputs of lgs_manager_insert (device int64), labels / labels_out device int64.
 * Dedup (first occurrence wins, surviving indices ascending) is lgs_manager_insert itself. */
int lgs_voxelize(const float *points, int64_t n, const double *affine, int batch, int32_t *coords, void *stream);
int lgs_label_vote(const int64_t *labels, int64_t n, const int64_t *unique_index, const int64_t *inverse,
                   int64_t n_unique, int64_t ignore_label, int64_t *labels_out, void *stream);

/* ---- PointGroup clustering (validation-time only) --------------------------------
 * replaces PG_OP.ballquery_batch_p + PG_OP.bfs_cluster
 *   /root/reference/downstream/insseg/lib/bfs/ops/src/bfs_cluster_kernel.cu:16-61, bfs_cluster.cpp:54-125,
 *   as called by downstream/insseg/lib/bfs/bfs.py:124-150.
 * Connected components of {(i,j): |p_i - p_j|^2 < radius^2 (float32, reference operation order), same batch, same
 * semantic label} through a radius-sized cell grid + lock-free union-find; component[i] = smallest point index of i's
 * component (= the point the reference's BFS starts it from, so clusters sorted by it come in the reference's order)
 * or -1 if the component has fewer than `threshold` points; *n_clusters (host) = kept components.  The reference's
 * per-point cap of 1000 neighbours / meanActive buffer is not reproduced (no neighbour lists are materialised).
 * Synchronises `stream` once.  batch_idx may be NULL (single scene). */
int64_t lgs_cluster_workspace_bytes(int64_t n);
int lgs_cluster(const float *xyz, const int32_t *batch_idx, const int32_t *semantic_label, int64_t n, float radius,
                int threshold, int32_t *component, int32_t *n_clusters, void *workspace, void *stream);

/* ---- fused softmax cross-entropy ----------------------------------------------------------------
 * replaces nn.CrossEntropyLoss(ignore_index=-1) on the [N,200] logits of the fine-tune step
 *   /root/reference/lib/train_test/pl_BaselineTrainer.py:94-99,350
 * One pass: loss_rows[n] (float32, 0 for ignored rows) and dlogits[n,c] = (softmax - onehot) * (*scale)
 * (same dtype as logits, zeros for ignored rows; rows whose label is outside [0, c) are treated as ignored).  Any class
 * count up to 512 (fp32) / 1024 (bf16) is accepted; counts that are not a multiple of the 16-byte width (20 ScanNet
 * classes in bf16) take element-wise accesses.  `scale` is a DEVICE float (e.g. 1 / #valid rows, times
 * the upstream gradient), so the mean reduction needs no host sync.  Either output may be NULL: the host
 * wrapper asks for the loss in the forward pass and for the gradient in the backward pass. */
int lgs_ce_forward_backward(const void *logits, int64_t n, int c, const int64_t *labels, int64_t ignore_index,
                            const float *scale, float *loss_rows, void *dlogits, int dtype, void *stream);
/* The same pass with a per-row gradient factor (ABI 13): dlogits[n,:] = (softmax - onehot) * (*scale) * row_scale[n].
 * This is the backward of nn.CrossEntropyLoss(reduction='none') -- what the fine-tune step runs when
 * --balanced_category_sampling True (/root/reference/scripts/train_models.sh:37, pl_BaselineTrainer.py:94,350-356):
 * loss_rows IS the reduction='none' output, row_scale the upstream gradient of sample_categories_for_balancing's masked mean
 * (lib/losses/utils.py:74-77: mask / N).  row_scale may be NULL (= lgs_ce_forward_backward). */
int lgs_ce_forward_backward_rows(const void *logits, int64_t n, int c, const int64_t *labels, int64_t ignore_index,
                                 const float *scale, const float *row_scale, float *loss_rows, void *dlogits, int dtype,
                                 void *stream);
/* head / common / tail statistics of per-point losses (ABI 13): what the trainer's three meters take from
 * sample_categories_for_balancing (/root/reference/lib/losses/utils.py:69-72, pl_BaselineTrainer.py:353-355) without its
 * three boolean-index gathers (= three host syncs).  group_of_class[n_classes] in {0,1,2} (anything else: not counted); rows whose
 * label is ignore_index or outside [0, n_classes) are skipped.  partial[partial_rows][6] (1 <= partial_rows <= 1024, overwritten):
 * per workgroup (sum, count) x 3 groups -- the caller adds the rows up (deterministic; no float atomics). */
int lgs_split_stats(const float *loss_rows, const int64_t *labels, int64_t n, const int32_t *group_of_class, int n_classes,
                    int64_t ignore_index, float *partial, int partial_rows, void *stream);
/* number of rows the loss above counts (label != ignore_index and inside [0, c)) -> *count (DEVICE int32, overwritten): the
 * denominator of the mean reduction (pl_BaselineTrainer.py:350, nn.CrossEntropyLoss(ignore_index) 'mean') without a host
 * sync and without a chain of elementwise / reduction launches over the label tensor. */
int lgs_ce_count_valid(const int64_t *labels, int64_t n, int c, int64_t ignore_index, int32_t *count, void *stream);

/* ---- focal loss and class-weighted cross-entropy (csrc/lgs_loss.hip, k_focal_fwd_bwd) -----------
 * replaces: the other two outcomes of loss_by_name(config.loss_type, ...) (lib/utils.py:112-118, pl_BaselineTrainer.py:96-99,
 *   downstream/insseg/lib/pl_Trainer.py:74): FocalLoss(alpha, gamma) (lib/losses/FocalLoss.py) and nn.CrossEntropyLoss(weight=...)
 * NEW SYMBOLS ONLY: LGS_ABI_VERSION stays 18; a library that lacks them lacks the capability.
 * Per row with label l, counted iff l != ignore_index and 0 <= l < c (the predicate of every loss entry above); p = softmax(z),
 * pt = p_l, u = 1 - pt, a = alpha[l] (alpha: DEVICE float[c], or NULL = all ones):
 *   loss_rows[n]   float32:  -a u^gamma log(pt);  0 for rows that are not counted
 *   dlogits[n, c]  dtype of logits:  coef (p_j - [j == l]) * (*scale) * row_scale[n],  coef = a (u^gamma - gamma pt u^(gamma-1) log(pt));
 *                  rows that are not counted are WRITTEN as zeros
 * gamma == 0 is nn.CrossEntropyLoss(weight=alpha, reduction='none') and its gradient; gamma >= 0 is required.  float32 arithmetic
 * whatever the dtype.  u is the exponential sum without the label's term over the full sum (no 1 - pt), log(pt) is log1p(-u) while
 * u < 1/2, and a row with u == 0 takes the limit: loss 0, coef = a for gamma == 0 and 0 otherwise -- finite where the reference's
 * autograd yields 0^(gamma-1) = NaN for gamma < 1.
 * scale, row_scale (NULL = ones), the two modes (either output may be NULL, not both), class limits (<= 512 fp32, <= 1024 bf16) and
 * the bytes moved are those of lgs_ce_forward_backward_rows, plus the 4-byte alpha[l] per row.  n == 0 launches nothing. */
int lgs_focal_forward_backward(const void *logits, int64_t n, int c, const int64_t *labels, int64_t ignore_index,
                               const float *alpha /* [c] or NULL */, float gamma, const float *scale,
                               const float *row_scale /* [n] or NULL */, float *loss_rows, void *dlogits, int dtype, void *stream);
/* sum of alpha[labels[i]] over the counted rows, the denominator of nn.CrossEntropyLoss(weight=alpha) 'mean':
 * partial[partial_rows] (1 <= partial_rows <= 1024, DEVICE float, overwritten), one float per workgroup -- the caller adds them up in
 * fixed order (deterministic; no float atomics; no host sync). */
int lgs_ce_weight_sum(const int64_t *labels, int64_t n, int c, int64_t ignore_index, const float *alpha,
                      float *partial, int partial_rows, void *stream);

/* ---- segmentation metrics (csrc/lgs_metrics.hip) ------------------------------------------------
 * replaces: what eval_step runs on the [N, 200] scores after the loss, in every training and validation step
 *   lib/train_test/pl_BaselineTrainer.py:357-378 (soutput.F.max(1)[1], softmax(soutput.F, 1), the confusion matrix behind
 *   precision / recall / IoU and their head / common / tail variants), pl_RepresentationTrainer.py:238-239
 * A NEW SYMBOL ONLY: LGS_ABI_VERSION stays 18; a library that lacks the symbol lacks the capability.
 * One pass over scores[n, c] (float32 / bf16, contiguous rows; class counts as lgs_ce_forward_backward: <= 512 fp32, <= 1024 bf16):
 *   pred[n]        int64, written for EVERY row: torch.max(scores, 1)[1] -- the lowest index among the maxima, the index of the
 *                  first NaN if the row has one, 0 for a row of -inf only
 *   prob[n, c]     float32 softmax of the values as stored, or NULL: then the pass writes 8 bytes per row and nothing else
 *   confmat[c, c]  int64, ACCUMULATED INTO and never cleared: confmat[labels[i]][pred[i]] += 1 for the rows with
 *                  labels[i] != ignore_index and 0 <= labels[i] < c (the `k` mask of lib/utils.py:97-99); every other row adds
 *                  nothing.  Integer sums (combined per half-wave, per workgroup in LDS, then 64-bit global atomics): the result
 *                  does not depend on the order, two calls give the same bits.
 * ignore_index may be any value, also a class index (255). */
int lgs_seg_metrics(const void *scores, int64_t n, int c, const int64_t *labels, int64_t ignore_index, int64_t *pred, float *prob,
                    int64_t *confmat, int dtype, void *stream);

/* ---- per-class average precision (csrc/lgs_ap.hip) -----------------------------------------------
 * replaces: AveragePrecision(num_classes, average=None)(prob, target) of every validation step
 *   (lib/train_test/pl_BaselineTrainer.py:380, downstream/insseg/lib/pl_Trainer.py:316) and sklearn's average_precision_score per class
 *   (downstream/insseg/lib/test.py:58-62, :215): C sorts of N scores, driven from the host
 * NEW SYMBOLS ONLY: LGS_ABI_VERSION stays 18; a library that lacks them lacks the capability.
 * ap_out[c] (DEVICE double, overwritten): sklearn's step-wise AP of every class, as
 *   AP_c = (1 / P_c) sum over the rows i with labels[i] == c of TP_c(s_i) / Rank_c(s_i),   s_i = prob[i, c],
 *   TP_c(s) = #{ j : labels[j] == c, prob[j, c] >= s },  Rank_c(s) = #{ j : prob[j, c] >= s } over ALL n rows
 * A row is a positive of its label's class iff labels[i] != ignore_index and 0 <= labels[i] < c; every other row is a negative of every
 * class.  A class without a positive gives NaN.  -0 ties with +0.  n == 0 is legal (all NaN, no workspace needed).
 * scores[n, c]: float32 / bf16, contiguous rows, class counts as lgs_seg_metrics (<= 512 fp32, <= 1024 bf16).  from_logits == 0: they
 * are the probabilities (any finite values rank).  from_logits != 0: prob is the fp32 softmax of the values as stored, with the very
 * expressions of lgs_seg_metrics' prob: the result equals, bit for bit, the call on that prob with from_logits == 0.
 * The positives are sorted (one radix sort of n 64-bit keys), every element of the matrix is counted against the sorted positives of
 * its column in one more pass, and the terms are added in fp64 in a fixed order: integer counts and one summation order, so two calls
 * give the same bits.  Enqueues on `stream`, never synchronises.  NaN scores are not supported: the result of a class they touch is
 * unspecified (nothing is read or written out of bounds).
 * workspace: lgs_ap_workspace_bytes(n, c) bytes (-1: c outside 1 .. 1024, n < 0, or the size query failed). */
int64_t lgs_ap_workspace_bytes(int64_t n, int c);
int lgs_average_precision(const void *scores, int64_t n, int c, const int64_t *labels, int64_t ignore_index, int from_logits,
                          double *ap_out /* [c] */, int dtype, void *workspace, void *stream);

/* ---- instance evaluation: proposal / ground-truth overlap tables (csrc/lgs_insteval.hip) ---------
 * replaces: the per-proposal host loop of Clustering.get_instances (downstream/insseg/lib/bfs/bfs.py:127-157: a dense [P, N] mask, one
 *   score_func over a boolean gather and three device -> host copies per proposal) and assign_instances_for_scan
 *   (downstream/insseg/datasets/evaluation/evaluate_semantic_instance.py:251-306: one [N] pass per (proposal, ground-truth instance))
 * NEW SYMBOLS ONLY: LGS_ABI_VERSION stays 18; a library that lacks them lacks the capability.
 * All pointers are DEVICE pointers.  Enqueues on `stream`, never synchronises.
 * Proposals in CSR form: member[offsets[q] .. offsets[q + 1]) are the point indices of proposal q (offsets[0] == 0, offsets[p] == m,
 *   ascending).  The members of one proposal are distinct (not checked); a point may belong to several proposals.
 * Ground truth: g = gt_ids[i] names an instance iff g != 0 and floor(g / 1000) is one of valid_class_ids[v] (ascending, all >= 1: a
 *   smaller one sets status bit 8).  Every other point is void; gt_ids == NULL: all of them are (the call then serves conf alone).
 * gt_id / gt_count [g_cap]: the distinct instance ids of the scene and their point counts; unused slots have gt_count == 0.  WHICH slot an
 *   id takes is unspecified (the compaction runs on the device); the map id -> (count, column of inter) is exact.  1 <= g_cap <= 4096.
 *   More than g_cap distinct ids set status bit 1: nothing is written out of bounds, the other outputs are unspecified.
 * inter[q, slot] ([p, g_cap]): members of q whose id is that slot's.  prop_void[q]: members of q that are void.
 *   prop_void[q] + sum(inter[q, :]) == offsets[q + 1] - offsets[q] whenever status == 0.
 * conf[q]: score_mode 1 = the maximum of scores[i, score_col[q]] over the members (bf16 widened exactly; the bits torch.max gives, NaN
 *   once a member is NaN); 2 = their mean, summed in fp64 per piece of at most 1024 members in a fixed tree, the pieces in order, rounded
 *   to fp32 once: two calls give the same bits.  An empty proposal, or a score_col outside [0, c) (status bit 4), gives NaN.
 *   score_mode 0 writes nothing to conf (scores, score_col, conf may be NULL).  scores[n, c]: float32 / bf16, contiguous rows.
 * A member outside [0, n) sets status bit 2 and is skipped.  p == 0, m == 0 and n == 0 are legal.  status is one int32, overwritten.
 * Integer sums only (LDS adds per workgroup, 32-bit global adds where a proposal spans several): the result does not depend on order.
 * workspace: lgs_inst_overlap_workspace_bytes(n, m, p, g_cap) bytes (-1: a negative size or g_cap outside 1 .. 4096). */
int64_t lgs_inst_overlap_workspace_bytes(int64_t n, int64_t m, int p, int g_cap);
int lgs_inst_overlap(const int32_t *member /* [m] */, const int32_t *offsets /* [p + 1] */, const int32_t *score_col /* [p] */, int p, int64_t m,
                     const int64_t *gt_ids /* [n] */, int64_t n, const int64_t *valid_class_ids /* [v] */, int v,
                     const void *scores /* [n, c] or NULL */, int c, int dtype, int score_mode, int g_cap, int64_t *gt_id /* [g_cap] */,
                     int32_t *gt_count /* [g_cap] */, int32_t *inter /* [p, g_cap] */, int32_t *prop_void /* [p] */, float *conf /* [p] */,
                     int32_t *status, void *workspace, void *stream);

/* ---- instance targets: per-instance table of a batch and the offset losses (csrc/lgs_insttarget.hip) ----
 * replaces: VoxelizationDataset.get_instance_info (downstream/insseg/datasets/dataset.py:280-304: per scene, on the host, one boolean
 *   mask over all points per instance id) with the masking of :336-341, the per-step concatenation and upload of centers and ids
 *   (downstream/insseg/lib/pl_Trainer.py:280-284) and the offset losses of :286-298 (about fifteen torch launches over [N, 3] per direction)
 * NEW SYMBOLS ONLY: LGS_ABI_VERSION stays 18; a library that lacks them lacks the capability.
 * All pointers are DEVICE pointers except masked_labels (HOST, read during the call).  Enqueues on `stream`, never synchronises.
 *
 * lgs_instance_info: coords[n, 4] int32 with the batch index in column 0, instance_ids[n] int64.  An instance is the pair (batch index,
 *   id): the same id in two scenes names two instances.  id == -1 names none; so does a point whose labels[i] equals one of the
 *   n_masked <= 32 masked_labels (n_masked == 0: labels may be NULL).  Any other id outside [0, 2^31) sets status bit 2, a negative
 *   batch index status bit 4; such a point is treated as -1.
 *   ids_out[n]: the ids after masking (-1 or the id).  slot[n]: the point's row of the table, -1 for none.
 *   key / count / bbox / center [inst_cap] / [inst_cap] / [inst_cap, 6] / [inst_cap, 3]: per instance (batch << 32) | id, its points, min
 *   xyz then max xyz, and its centre.  Unused rows hold key -1, count 0, zeros.  WHICH row an instance takes is unspecified, but it
 *   depends on the set of instances alone: two calls on the same points give the same rows.  The map instance -> (count, box, centre)
 *   is exact: the three coordinate sums are signed 64-bit integers, count and box are integers, and
 *   center = (float)((double)sum / (double)count) -- what numpy's xyz.mean(0) stored into a float32 row gives.
 *   centers[n, 3] (may be NULL): center[slot] per point, -1 on the rows without an instance: the reference's array.
 *   status: one int32, overwritten.  Bit 1: more than inst_cap distinct instances -- nothing is written out of bounds, the instances
 *   beyond the capacity get slot -1, the other outputs are unspecified.  1 <= inst_cap <= 65536.  n == 0 is legal.
 *   Integer atomics only, folded per workgroup in LDS before they reach global memory; the result does not depend on order.
 *   workspace: lgs_instance_info_workspace_bytes(n, inst_cap) bytes (-1: n outside 0 .. 2^31 - 1 or inst_cap outside 1 .. 65536); it
 *   depends on inst_cap alone.
 *
 * lgs_offset_loss_forward: pt_offsets[n, 3] float32 / bf16 (widened exactly), coords and slot as above, center = the table.  Per row with
 *   slot >= 0, in fp32 and the reference's order: gt = (center[slot] - xyz) * voxel_size; dist = sum |po - gt|;
 *   dir = -sum (gt / (|gt| + 1e-8)) * (po / (|po| + 1e-8)).  partial[partial_rows, 3] (fp64, 1 <= partial_rows <= 1024 = the grid):
 *   per workgroup the sums of dist, of dir and the number of such rows, folded in a fixed tree; one more launch adds the rows in
 *   a fixed tree and writes *norm_loss = sum dist / (valid + 1e-6), *dir_loss = sum dir / (valid + 1e-6), *valid = the count, each
 *   rounded to fp32 once.  No float atomics: two calls give the same bits.  n == 0 gives 0, 0, 0.
 * lgs_offset_loss_backward: d_pt_offsets[n, 3] in `dtype` =
 *     (*g_norm / den) * sign(po - gt) + (*g_dir / den) * d dir / d po,   den = *valid + 1e-6,   sign(0) = 0,
 *   d dir / d po = -u / D + (u . po / D) po / (D |po|) with u = gt / (|gt| + 1e-8), D = |po| + 1e-8 and the second term absent at
 *   po == 0 (torch's zero subgradient of the norm); zero on the rows without an instance.  valid, g_norm, g_dir: one DEVICE float
 *   each (valid: what the forward wrote).  Neither direction reads or writes an [n, 3] array but pt_offsets and d_pt_offsets. */
int64_t lgs_instance_info_workspace_bytes(int64_t n, int inst_cap);
int lgs_instance_info(const int32_t *coords /* [n, 4] */, const int64_t *instance_ids /* [n] */, const int64_t *labels /* [n] or NULL */,
                      int64_t n, const int64_t *masked_labels /* HOST [n_masked] */, int n_masked, int inst_cap, int64_t *ids_out /* [n] */,
                      int32_t *slot /* [n] */, int64_t *key /* [inst_cap] */, int32_t *count /* [inst_cap] */, int32_t *bbox /* [inst_cap, 6] */,
                      float *center /* [inst_cap, 3] */, float *centers /* [n, 3] or NULL */, int32_t *status, void *workspace, void *stream);
int lgs_offset_loss_forward(const void *pt_offsets /* [n, 3] */, const int32_t *coords /* [n, 4] */, const int32_t *slot /* [n] */,
                            const float *center /* [inst_cap, 3] */, int64_t n, float voxel_size, int dtype, double *partial /* [partial_rows, 3] */,
                            int partial_rows, float *norm_loss, float *dir_loss, float *valid, void *stream);
int lgs_offset_loss_backward(const void *pt_offsets /* [n, 3] */, const int32_t *coords /* [n, 4] */, const int32_t *slot /* [n] */,
                             const float *center /* [inst_cap, 3] */, int64_t n, float voxel_size, int dtype, const float *valid,
                             const float *g_norm, const float *g_dir, void *d_pt_offsets /* [n, 3] */, void *stream);

/* ---- supervised point-contrastive loss (csrc/lgs_supcon.hip) -------------------------------------
 * replaces: PointSupConLoss.forward (lib/losses/PointSupConLoss.py:74-154), the third embedding criterion of
 *   BaselineTrainerModule.init_criterions (lib/train_test/pl_BaselineTrainer.py:92-108): per class of the batch three device -> host
 *   copies and two np.random.choice calls over all N points in a joblib pool, then [N, P, C] + [N, K, C] fp32 sample tensors and a bmm
 * NEW SYMBOLS ONLY: LGS_ABI_VERSION stays 18; a library that lacks them lacks the capability.
 * A row is counted iff its label is not ignore_label and inside [0, n_labels).  P = p and K = k are 1 .. 8 each.  A sample index
 * outside [0, n) (the sampler writes -1) is "no sample": the all-zero row.  n == 0 launches nothing.  No LDS, atomics or workspace.
 *
 * lgs_supcon_sample: pos_idx[n, p], neg_idx[n, k] (int64) from tables the caller builds with device ops (all DEVICE int64):
 *   order[n]            row numbers sorted (stably) by the key 2 * label + (not eligible), rows that are not counted last
 *   seg_start[n_labels] first position of class c in `order`;  cls_count[c] its points;  elig_count[c] = m[c], the eligible ones
 *                       (counted and, with predictions, correctly predicted), which come first in the segment
 *   cum[n_labels, n_labels]  INT64 cumulative sums along each row of w[u, c] = hist[u, c] * m[c] * [c != u], hist >= 0
 *   A positive is order[seg_start[u] + U(cls_count[u])] for the row's class u (uniform, with replacement, the row itself and
 *   mispredicted points included, :120).  A negative draws x = U(cum[u, L-1]), takes the first class c with cum[u, c] > x (binary
 *   search; a class of weight 0 owns no integer and is never drawn) and then order[seg_start[c] + U(m[c])] -- the two-level form of
 *   np.random.choice(N, p = hist[u, label_j] * eligible_j / sum) (:124-139).  A row that is not counted gets -1 everywhere, a row whose
 *   total weight is 0 gets -1 negatives.  U(t) = high 64 bits of r * t with r 64 random bits from Philox-4x32-10, key = seed,
 *   counter = (row, slot): the indices depend on (seed, row, slot) only.  `seed` is a HOST integer.
 *
 * lgs_supcon_forward: one wavefront per row reads feat[n, c] (float32 / bf16; 16-byte loads when c * elemsize and the base address
 *   are multiples of 16, element loads otherwise) and its p + k sampled rows: (1 + p + k) * n * c * elemsize bytes.  fp32 arithmetic.
 *   LGS_SUPCON_COS: sim[n, p + k] = <a^, b^_j>, x^ = x / max(|x|, 1e-12);   d = 1 - mean_j sim_j  over the p / the k slots
 *   LGS_SUPCON_L2:  sim[n, p + k] = sqrt(sum_c (a_c - b_jc)^2 + 1e-7), on the differences;   d = mean_j sim_j
 *   d_pos[n], d_neg[n], sim (all float32) are 0 for rows that are not counted (:70);  inv_norm[n] = 1 / max(|a_n|, 1e-12) for EVERY row.
 * lgs_supcon_backward: grad_feat[n, c] (dtype of feat; one round-to-nearest-even store for bf16) from the upstream g_dpos[n],
 *   g_dneg[n] (float32, either may be NULL = zeros) and the forward's sim / inv_norm.  The sampled rows are constants (:77):
 *   COS: gf = 1/|a| * sum_j gs_j (b^_j - s_j a^), gs_j = -g_dpos / p | -g_dneg / k, b^_j = b_j * inv_norm[idx_j] (|a| <= 1e-12: the
 *        gradient of a / 1e-12, no projection term);   L2: gf = sum_j g_j (a - b_j) / (S sim_j), S = p | k.
 *   Rows that are not counted are WRITTEN as zeros.  Reads as the forward, writes n * c * elemsize. */
int lgs_supcon_sample(const int64_t *labels, int64_t n, int n_labels, int64_t ignore_label, const int64_t *cum,
                      const int64_t *order, const int64_t *seg_start, const int64_t *cls_count, const int64_t *elig_count,
                      int p, int k, int64_t seed, int64_t *pos_idx, int64_t *neg_idx, void *stream);
int lgs_supcon_forward(const void *feat, int64_t n, int c, const int64_t *labels, const int64_t *pos_idx, int p,
                       const int64_t *neg_idx, int k, int64_t ignore_label, int n_labels, int distance, float *d_pos,
                       float *d_neg, float *sim, float *inv_norm, int dtype, void *stream);
int lgs_supcon_backward(const void *feat, int64_t n, int c, const int64_t *labels, const int64_t *pos_idx, int p,
                        const int64_t *neg_idx, int k, int64_t ignore_label, int n_labels, int distance, const float *sim,
                        const float *inv_norm, const float *g_dpos, const float *g_dneg, void *grad_feat, int dtype,
                        void *stream);

/* ---- train-time augmentation chain (csrc/lgs_augment.hip) ---------------------------
 * replaces: the numpy / scipy transforms the reference runs in DataLoader workers (lib/transforms.py, wired up in
 *   lib/dataset.py:355-389): ElasticDistortion before the voxeliser, RandomHorizontalFlip, ChromaticAutoContrast,
 *   ChromaticTranslation, ChromaticJitter and ChromaticScale after it, plus the voxeliser's per-scene rigid matrix.
 * NEW SYMBOLS ONLY: LGS_ABI_VERSION stays 18; a library that lacks them lacks the capability.
 * A batch is b <= LGS_AUG_MAX_SCENES scenes concatenated; rows of one scene are contiguous and scene_offsets[b + 1] (DEVICE int64,
 * scene_offsets[0] = 0, non-decreasing, scene_offsets[b] = n) says where each begins.  An empty scene is legal everywhere.  Nothing
 * here reads device memory back except lgs_aug_status.  Per-scene parameters are HOST arrays, passed to the kernels by value.
 *
 * lgs_aug_bounds: bounds[b, 6] = per scene (min of 3 columns, max of 3 columns), DEVICE, the table's own 32-bit type.
 *   LGS_AUG_F32X3: table = float32 [n, 3]; scene_offsets is READ.  Floats are compared through an order-preserving integer key
 *                  (-0.0 sorts below +0.0); an empty scene gets (+inf, -inf).
 *   LGS_AUG_I32X4: table = int32 [n, 4], scene id in column 0 (ascending), columns 1..3 reduced; scene_offsets is WRITTEN first
 *                  (derived from column 0) and may be handed to the calls below.  An empty scene gets (INT32_MAX, INT32_MIN).
 *   Reduced in the wave, then the workgroup; one global atomic min / max per workgroup, scene and column.
 *
 * lgs_elastic_distort: ONE stage of ElasticDistortion.elastic_distortion(granularity, magnitude) on points[n, 3] in place, for every
 *   scene whose bit is set in apply_mask.  bounds_in[b, 6]: the cloud's bounds (lgs_aug_bounds, or the previous stage's
 *   bounds_out).  Per scene, on the device: noise_dim = ((max - min) // granularity) + 3 in float32 as numpy does it; a grid of more
 *   than max_cells cells leaves the scene untouched and sets bit `scene` of *status (DEVICE int32, OR-ed, never cleared here).
 *   Noise: noise (DEVICE float32 [b, max_cells * 3], each scene's [dx, dy, dz, 3] block packed at the start of its slot) if not NULL,
 *   else N(0, 1) by Box-Muller from Philox-4x32-10 with counter = (cell, component, stage, seed >> 32) and key = (seed & 2^32-1,
 *   scene_seeds[scene]): a scene's field does not depend on the batch around it.  scene_seeds: HOST int32[b] or NULL (zeros).
 *   Field: two rounds of zero-padded 3-tap box blurs along x, y, z = per axis T^2 of the d x d tridiagonal(1/3) matrix, weights
 *   count(i, j) / 9 (the interior row is [1,2,3,2,1]/9, the edge rows are smaller), applied as one 125-tap pass with exact integer
 *   weights.  Apply: trilinear sample on the axes min - g + i g (0 outside), p += sample * magnitude, evaluated in double and rounded
 *   once.  bounds_out[b, 6] (must not alias bounds_in) = bounds of the cloud after this stage, for the next one.
 *   workspace: lgs_elastic_workspace_bytes(b, max_cells) bytes.
 *
 * lgs_voxelize_batched: lgs_voxelize with one affine per scene (affines: HOST double [b, 12]); column 0 = batch_base + scene.
 * lgs_coords_flip_shift: coords int32 [n, 4] in place: axis a of scene s becomes max - c where bit a of flip_axes[s] (HOST int32[b])
 *   is set, max = bounds[s, 3 + a] (lgs_aug_bounds, LGS_AUG_I32X4); then shift[a] (HOST int32[3] or NULL) is added in every scene.
 * lgs_color_augment: colors float32 [n, 3] in place, per scene by lgs_color_scene, in the reference's order:
 *   LGS_COLOR_AUTOCONTRAST  f = (1 - blend) f + blend (f - lo) 255 / (hi - lo), lo / hi = bounds[s] (lgs_aug_bounds over these rows).
 *                           A channel with hi == lo is left unblended (the reference yields inf / NaN there): the one deviation.
 *   LGS_COLOR_TRANSLATION   f = clip(f + translation, 0, 255)
 *   LGS_COLOR_JITTER        f = clip(f + jitter_std 255 z, 0, 255), z = noise[n, 3] (DEVICE float32) if not NULL, else Philox with
 *                           counter = (row within the scene (64 bit), channel, LGS_AUG_STAGE_COLOR ^ seed >> 32), key as above with `seed`
 *   then f *= scale, then f = f / 255 - 0.5 if normalize.
 * lgs_aug_status: copies *status to the host and SYNCHRONISES the stream (the lgs_manager_check pattern).
 * lgs_debug_philox: out[n, 4] = Philox-4x32-10(counter[n, 4], key = (key & 2^32-1, key >> 32)), DEVICE int32 words (tests). */
#define LGS_AUG_MAX_SCENES 32
#define LGS_AUG_F32X3 0
#define LGS_AUG_I32X4 1
#define LGS_AUG_STAGE_COLOR 16
#define LGS_AUG_STAGE_PASTE 17          /* the tail-instance paste's trial draws (below) */
#define LGS_AUG_STAGE_DROPOUT 18        /* RandomDropout's row keys (below) */
#define LGS_AUG_STAGE_INSTSHIFT 19      /* the per-instance colour / scale decisions (below) */
#define LGS_PASTE_MAX_SLOTS 1024
#define LGS_PASTE_SLOT_COLS 6
#define LGS_PASTE_SCENE_COLS 4
#define LGS_COLOR_AUTOCONTRAST 1
#define LGS_COLOR_TRANSLATION 2
#define LGS_COLOR_JITTER 4
typedef struct lgs_color_scene {
  int32_t flags;          /* LGS_COLOR_* */
  int32_t seed;           /* the scene's Philox key word */
  float blend;
  float translation[3];
  float jitter_std;
  float reserved;
} lgs_color_scene;
int lgs_aug_bounds(const void *table, int64_t n, int form, int64_t *scene_offsets, int b, void *bounds, void *stream);
int64_t lgs_elastic_workspace_bytes(int b, int64_t max_cells);
int lgs_elastic_distort(float *points, int64_t n, const int64_t *scene_offsets, int b, const float *bounds_in, double granularity,
                        double magnitude, int64_t seed, const int32_t *scene_seeds, int apply_mask, int stage, const float *noise,
                        int64_t max_cells, void *workspace, float *bounds_out, int32_t *status, void *stream);
int lgs_voxelize_batched(const float *points, int64_t n, const int64_t *scene_offsets, int b, const double *affines,
                         int batch_base, int32_t *coords, void *stream);
int lgs_coords_flip_shift(int32_t *coords, int64_t n, const int64_t *scene_offsets, int b, const int32_t *bounds,
                          const int32_t *flip_axes, const int32_t *shift, void *stream);
int lgs_color_augment(float *colors, int64_t n, const int64_t *scene_offsets, int b, const float *bounds,
                      const lgs_color_scene *scenes, float scale, int normalize, int64_t seed, const float *noise, void *stream);
int lgs_aug_status(const int32_t *status, int *flags, void *stream);
int lgs_debug_philox(const int32_t *counters, int64_t n, int64_t key, int32_t *out, void *stream);

/* ---- class-balanced tail-instance paste (csrc/lgs_paste.hip) -------------------------------------
 * replaces: ScannetVoxelizationDataset.add_instances_to_cloud (lib/datasets/scannet.py:143-241), the reference's
 *   --sample_tail_instances: per scene a height map with a 5 x 5 maximum filter, per pasted instance up to `trials` placement
 *   trials against the scene's instance boxes, then the rotation M_r of every row.  The dedup that follows is the caller's.
 * NEW SYMBOLS ONLY: LGS_ABI_VERSION stays 18; a library that lacks them lacks the capability.
 * A batch is b <= LGS_AUG_MAX_SCENES scenes, coords int32 [n, 4] with the scene index 0 .. b - 1 in column 0 (ascending) and
 * floor(M_v p) in columns 1..3, feats float32 [n, 3], labels int64 [n].  A SLOT is one (scene, instance) pair, at most
 * LGS_PASTE_MAX_SLOTS per call, slots of a scene adjacent and in paste order; the instances' rows, slot after slot, are the
 * inst_rows INSTANCE ROWS.  The bank is bank_points / bank_colors float32 [bank_rows, 3] and bank_labels int64 [bank_rows], world
 * units.  Every table is DEVICE memory, filled by the host (one upload serves them all):
 *   slot_table    int64 [slots + 1, LGS_PASTE_SLOT_COLS] = (first bank row, first instance row, first output row, scene, index of
 *                 the instance within its scene, rows); every slot has at least one row; record `slots` holds inst_rows in column 1.
 *   slot_affines  double [slots, 12]: the instance's own M_r M_v (the reference voxelises each instance with augmentation on).
 *   scene_table   int64 [b + 1, LGS_PASTE_SCENE_COLS] = (first output row of the scene's own rows, first box, the scene's Philox
 *                 key word, first input row); record b holds n_boxes in column 1 and n in column 3.  An empty scene has no slots.
 *   scene_xforms  double [b, 13] = (the scalar of M_v, then M_r as [3, 4]).
 *   boxes         double [n_boxes, 6] = world-space (min corner, max corner); a trial compares against round(corner * scalar).
 * Steps (float64 wherever the reference computes in float64; integer atomics only, so two calls give the same bits):
 *   instance voxels  floor(M p) with lgs_voxelize_batched's arithmetic.  A row is FIRST if it is the lowest row of its (slot, voxel),
 *                    found through an open-addressing table of packed keys (18 bits per coordinate).
 *   statistics       over first rows per slot: min, max, int64 sum, count -> dims = max - min + 1, mean = trunc(sum / count).
 *   height map       per scene int32 [dim_x, dim_y] over the bounds of its rows (lgs_aug_bounds), z_min where no row lies.
 *   placement        trial t: (x, y) = trial_draws[slot, t] (DEVICE int32 [slots, trials, 2], clamped into the scene's bounds) if
 *                    not NULL, else x = x_min + (w0 dim_x >> 32), y likewise with w1, (w0, w1) from Philox-4x32-10 with counter =
 *                    (t, index within the scene, LGS_AUG_STAGE_PASTE, seed >> 32) and key = (seed & 2^32-1, scene key word).
 *                    h = max of the map over the 5 x 5 window clamped to the map (= scipy's maximum_filter(size=5), reflect);
 *                    centroid = (x, y, trunc(h + dims_z / 2.0)); the trial fails if any box of the scene intersects
 *                    centroid -+ dims / 2.0 (inclusive on all six comparisons).  The first trial that does not fail wins; if all
 *                    fail the last trial's centroid is used.  placement int32 [slots, 4] = (winning trial, `trials` if all failed,
 *                    -1 if the scene was not pasted; centroid).
 *   output           per scene its own rows, then its instances in slot order, n + inst_rows rows: coords_out = (scene,
 *                    floor(M_r c)), c = the scene row, or voxel - mean + centroid; feats_out / labels_out copied alongside.
 * A scene whose map has more than max_map_cells (1 .. 2^26) cells, or with an instance voxel outside [-2^17, 2^17), is NOT pasted:
 *   bit `scene` of *status (DEVICE int32, OR-ed, never cleared here; read with lgs_aug_status) is set and its instance rows are
 *   written as copies of the scene's first row, which the dedup drops.
 * workspace: lgs_paste_workspace_bytes(b, slots, inst_rows, max_map_cells) bytes (0 = bad shape).  Nothing is read back. */
int64_t lgs_paste_workspace_bytes(int b, int slots, int64_t inst_rows, int64_t max_map_cells);
int lgs_paste_instances(const int32_t *coords, const float *feats, const int64_t *labels, int64_t n, int b, const float *bank_points,
                        const float *bank_colors, const int64_t *bank_labels, int64_t bank_rows, const int64_t *slot_table,
                        const double *slot_affines, int slots, int64_t inst_rows, const int64_t *scene_table,
                        const double *scene_xforms, const double *boxes, int64_t n_boxes, const int32_t *trial_draws, int trials,
                        int64_t seed, int64_t max_map_cells, void *workspace, int32_t *coords_out, float *feats_out,
                        int64_t *labels_out, int32_t *placement, int32_t *status, void *stream);

/* ---- RandomDropout: an exact-count uniform row subset per scene (csrc/lgs_dropout.hip) -----------
 * replaces: RandomDropout (lib/transforms.py:172-195, downstream/insseg/datasets/transforms.py:145-159): on the voxel rows of one
 *   scene, np.random.choice(N, int(N * (1 - ratio)), replace=False) and the gathers by it.
 * NEW SYMBOLS ONLY: LGS_ABI_VERSION stays 18; a library that lacks them lacks the capability.
 * A batch is 1 <= b <= LGS_AUG_MAX_SCENES scenes of n rows in all, scene_offsets DEVICE int64 [b + 1] as above (entries are clamped
 * into a non-decreasing table on [0, n]).  Scene s has n_s rows; bit s of apply_mask says whether it drops rows.
 *   count      k_s = floor(n_s * keep) in IEEE double, keep in (0, 1] = the host's 1 - ratio; a scene whose bit is clear keeps n_s.
 *   key        row i (0-based within its scene) has the uint32 key = word 0 of the Philox-4x32-10 block with counter
 *              (i & 2^32-1, i >> 32, 0, LGS_AUG_STAGE_DROPOUT ^ seed >> 32) and key (seed & 2^32-1, scene_seeds[s]); scene_seeds: HOST
 *              int32 [b] or NULL (zeros).  keys (DEVICE int32 [n], read as uint32, indexed by the batch row) replaces the generator
 *              when not NULL (teacher-forced; the only way to meet equal keys on purpose).
 *   selection  the k_s rows that are smallest under the lexicographic order (key, i): equal keys resolve towards the lower row.
 *   output     rows_out (DEVICE int64, capacity n): scene after scene the kept rows in ascending order, as g (the row's index in the
 *              batch), or through[g] when through (DEVICE int64 [n]) is not NULL; offsets_out DEVICE int64 [b + 1]: where each
 *              scene's kept rows begin, offsets_out[b] = the number of rows written.  k_s and n_s may be 0.
 * Two deviations from the reference: it returns the rows in np.random.choice's permutation order, this returns the same kind of set in
 * ascending order; and equal 32-bit keys resolve towards the lower row, which touches the threshold key only (a probability of order
 * n_s / 2^32 per scene that the threshold key is shared at all).
 * How: a three-digit radix select (11 + 11 + 10 bits) over keys that are regenerated in every pass -- the selection reads no row data
 * -- with per-scene histograms summed by integer atomics, then a count per tile, one scan per scene and a stable compaction by
 * ballot and popcount.  Dependent steps are separate launches; the result does not depend on any launch grid, and two calls give the
 * same bits.  Nothing is read back.  workspace: lgs_dropout_workspace_bytes(n, b) bytes (0 = bad shape: n < 0, n > 2^40, b out of
 * range); the call initialises what it reads of it. */
int64_t lgs_dropout_workspace_bytes(int64_t n, int b);
int lgs_dropout_select(const int64_t *scene_offsets, int64_t n, int b, unsigned int apply_mask, double keep, int64_t seed,
                       const int32_t *scene_seeds, const int32_t *keys, const int64_t *through, void *workspace, int64_t *rows_out,
                       int64_t *offsets_out, void *stream);

/* ---- per-instance colour and scale shifts (csrc/lgs_instshift.hip) -------------------------------
 * replaces: ScannetVoxelizationDataset.augment_instances (lib/datasets/scannet.py:243-319, instance_augmentation == 'raw') with
 *   InstanceAugmentation (lib/transforms.py:288-382): per tail instance of a scene one boolean mask over the cloud, a colour or a
 *   scale shift with the attribute it is named by, and the np.delete / np.vstack that moves every tail instance to the end.
 * NEW SYMBOLS ONLY: LGS_ABI_VERSION stays 18; a library that lacks them lacks the capability.
 * A batch is 1 <= b <= LGS_AUG_MAX_SCENES scenes of n rows in all (n < 2^31 - 1), scene_offsets DEVICE int64 [b + 1] as above (entries
 * are clamped into a non-decreasing table on [0, n]); points / colors DEVICE float32 [n, 3] (colours in 0 .. 255), labels /
 * instance_ids DEVICE int64 [n]; scene_bounds DEVICE float32 [b, 6], lgs_aug_bounds over `points`.  tail_labels: HOST int64
 * [n_tail], n_tail <= 256, any order.
 *   segment    the rows of one scene that share (label in tail_labels, instance id), 0 <= id < 2^31.  A row with id -1 or an id
 *              outside that range is in no segment (the reference would group such rows: a deviation); the latter sets bit `scene`
 *              of status[1].  Segments are ordered by (scene, label, id).
 *   decision   one per segment: attribute 0 (nothing), 1 .. 6 (colour: Red, Green, Blue, Yellow, Dark, Bright), 7 / 8 (scale up /
 *              down) and a factor f.  forced_keys (DEVICE int64 [n_forced, 3] = (scene, label, id)) with forced_attr (DEVICE int32)
 *              and forced_factor (DEVICE double) replaces the draws when not NULL; a segment it does not list gets 0.  Otherwise the
 *              Philox-4x32-10 block with counter (id, label & 2^32-1, label >> 32, LGS_AUG_STAGE_INSTSHIFT ^ seed >> 32) and key
 *              (seed & 2^32-1, scene_seeds[s]) (scene_seeds: HOST int32 [b] or NULL), u_k = word_k / 2^32 in double:
 *              u_0 < color_prob -> colour 1 + floor(6 u_2); else u_1 < scale_prob -> up iff 2 u_2 > 1, f = 1 + (h - 1) u_3 with
 *              h = min(1.5, min over the axes of fl32(scene extent / segment extent), inf and NaN quotients skipped), or down,
 *              f = 0.5 + 0.5 u_3 (double, every operation rounded).
 *   colour     Dark trunc(c 0.5); Bright trunc(255 - (255 - c) / 2), fp32.  The four hues, hue_as_written != 0 (the reference's
 *              hsv_to_rgb casts values in [0, 1] to uint8): a channel is 255 iff the row's maximum is 255 and (the channel is in the
 *              hue's set {r}, {g}, {b}, {r, g} or r == g == b), else 0.  hue_as_written == 0: the set's channels get max(r, g, b),
 *              the others min(r, g, b).
 *   scale      p' = fl32(fl32(p fl32(f)) + fl32(c fl32(1 - f))), c = ((lo_x + hi_x) / 2, (lo_y + hi_y) / 2, lo_z) over the segment's
 *              rows before scaling, 1 - f in double.
 *   output     per scene: the rows of no segment, ascending, then the segments in order, each with its rows ascending (the
 *              reference's row order; the dedup that follows lets the first occurrence win).  order (DEVICE int64 [n]) = the
 *              source row of every output row; points_out / colors_out [n, 3], labels_out int64 [n, 2] = (label, attribute),
 *              instances_out int64 [n].  Outputs may not alias inputs.
 * status: DEVICE int32 [2] of scene bits, OR-ed, never cleared here (read with lgs_aug_status, word by word).  status[0]: scenes
 *   left exactly as they were (identity order, attribute 0) because they hold a segment whose rank among the batch's segments is
 *   >= seg_cap (1 .. 65536); every scene, if the batch has more distinct segments than the table's 2^k >= 2 seg_cap entries.
 * How: per-workgroup LDS tables folded into one open-addressing table by integer atomics (count, order-preserving min / max keys),
 *   ranks by counting keys, one stable radix sort of (scene, rank) keys over the bits they use, one streaming gather.  The result
 *   does not depend on any launch grid, two calls give the same bits, nothing is read back.
 * workspace: lgs_instance_shift_workspace_bytes(n, b, seg_cap) bytes (0 = bad shape, or no device to size rocPRIM's temporary
 *   for: the query launches nothing but asks the current device); the call initialises what it reads of it. */
int64_t lgs_instance_shift_workspace_bytes(int64_t n, int b, int seg_cap);
int lgs_instance_shift(const float *points, const float *colors, const int64_t *labels, const int64_t *instance_ids, int64_t n,
                       const int64_t *scene_offsets, int b, const float *scene_bounds, const int64_t *tail_labels, int n_tail,
                       double color_prob, double scale_prob, int64_t seed, const int32_t *scene_seeds, const int64_t *forced_keys,
                       const int32_t *forced_attr, const double *forced_factor, int n_forced, int hue_as_written, int seg_cap,
                       void *workspace, float *points_out, float *colors_out, int64_t *labels_out, int64_t *instances_out,
                       int64_t *order, int32_t *status, void *stream);

/* ---- furthest point sampling over segments: the limited-annotation subsets (csrc/lgs_fps.hip) ----
 * replaces: furthest_point_sample (lib/ext/pointnet2/_ext_src/src/sampling_gpu.cu:75-178) as lib/datasets/preprocessing/
 *   scannet_long.py:98-109 calls it, once per annotated instance of a scene with max(5, round(ratio * n)) samples.
 * NEW SYMBOLS ONLY: LGS_ABI_VERSION stays 18; a library that lacks them lacks the capability.
 * points DEVICE float32 [n, 3], 0 <= n < 2^31 - 1.  Segment q of 0 <= s <= 2^20 owns the positions [seg_offsets[q], seg_offsets[q + 1])
 * of a sequence of length n (seg_offsets DEVICE int64 [s + 1]; entries are clamped into a non-decreasing table on [0, n]); position u
 * is row through[u] of points (through DEVICE int64 [n]; a value outside [0, n) is clamped into it), row u when through is NULL.
 *   segment    n_q points p[0 .. n_q) in position order, m_q samples.  Point k is eligible iff (x x + y y) + z z > 1e-3f (the reference's
 *              skip of near-origin points, as written), every point if skip_origin == 0.  t[k] = 1e10f, out[0] = 0.  Round
 *              j = 1 .. m_q - 1 with o = out[j - 1]: for every eligible k, d = ((xk - xo)^2 + (yk - yo)^2) + (zk - zo)^2 with every
 *              operation rounded to fp32 in this order and no contraction, t[k] = min(d, t[k]); out[j] = the eligible k with the
 *              largest t[k], the smallest such k on a tie, 0 if no point is eligible.  m_q > n_q is legal and repeats points.
 *              Non-finite coordinates: the selection is unspecified, nothing is read or written out of bounds, the call ends.
 *   count      m_q = counts[q] (DEVICE int32 [s], negative = 0) when counts is not NULL; else fixed_count when >= 0; else the recipe's
 *              rule on the device, max(min_points, (int)rint(ratio * n_q)) in IEEE double with round-half-even (Python's
 *              round(ratio * n)), 0 <= ratio <= 1.  n_q == 0 forces m_q = 0; m_q is capped at LGS_FPS_MAX_SAMPLES.
 *   output     either or both.  idx_out DEVICE int32: out[0 .. m_q) of segment q, LOCAL to the segment, at out_offsets[q] (DEVICE
 *              int64 [s]), or at q * fixed_count when out_offsets is NULL (a fixed count only).  rank_out DEVICE int32 [n], per ROW:
 *              the first round that chose the row, -1 for every other row of the table; all n entries are written (a row that
 *              several segments share takes the smallest round).
 * Deviation: the reference resolves an exact tie in a round's maximum by its block-strided reduction tree, so its choice depends on
 * its block size; here a tie goes to the smallest index.  The two agree on every input without an exact tie and after exhaustion.
 * How: one wave (n_q <= LGS_FPS_WAVE_MAX) or one workgroup per segment; the state in registers up to LGS_FPS_GROUP16_MAX points, in
 * the workspace beyond; per round one wave maximum of a 64-bit key (t's bits, ~k) and at most one barrier.  The result does not
 * depend on tier, grid or workgroup size, two calls give the same bits, nothing is read back.  workspace:
 * lgs_fps_workspace_bytes(n, s) bytes (0 = bad shape); the call initialises what it reads of it. */
#define LGS_FPS_WAVE_MAX 256
#define LGS_FPS_GROUP4_MAX 2048
#define LGS_FPS_GROUP16_MAX 8192
#define LGS_FPS_MAX_SAMPLES (1 << 24)
int64_t lgs_fps_workspace_bytes(int64_t n, int64_t s);
int lgs_fps_segments(const float *points, int64_t n, const int64_t *through, const int64_t *seg_offsets, int64_t s,
                     const int32_t *counts, int fixed_count, double ratio, int min_points, int skip_origin,
                     const int64_t *out_offsets, int32_t *idx_out, int32_t *rank_out, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LGS_ENGINE_H */
