// lgs_common.h -- internal helpers shared by the engine's translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/lgs_engine.h"
#include "lgs_idioms.h"

struct lgs_kmap;
struct lgs_segmap;

namespace lgs {

void set_error(const std::string &msg);

#define LGS_HIP(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) {                                                                        \
      lgs::set_error(std::string(#expr) + " failed: " + hipGetErrorString(_e) + " (" __FILE__ ":" + \
                     std::to_string(__LINE__) + ")");                                              \
      return 1;                                                                                    \
    }                                                                                              \
  } while (0)

#define LGS_REQUIRE(cond, msg)                                                     \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      lgs::set_error(std::string(msg) + " [" #cond "] (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
      return 2;                                                                    \
    }                                                                              \
  } while (0)

// ---- tuning table + dispatch counters (lgs_tuning.hip)
enum Tune {
  T_WW_MIN_ROWS, T_WW_RANGE, T_WGRAD_WIDE, T_BN_FUSED, T_BN_FUSED_MAX_MB, T_BN_FUSED_FWD_MAX_MB, T_BN_FUSED_BLOCKS, T_PS_CUS, T_PS_WIDE3, T_WGRAD_PS,
  T_MASK_WINDOW, T_CONV_SPLIT, T_SMALL_CFG, T_WIDE_GC64, T_ARENA_DBG, T_CONV_WIDE, T_MASK_ORDER,
  T_BN_FOLD, T_BN_FOLD_MAX_MB, T_BN_FOLD_PARTS, T_BN_FOLD_GRID, T_FP32_SPLIT, T_BLOCK_WGRAD_LATE, T_WGRAD_F32_LDS, T_WIDE_SCHED, T_HEAD_TILE, T_POINTWISE,
  T_INSTANCE_NORM, T_METRICS_BLOCKS, T_SUPCON_FUSED, T_BN_PAIR, T_MAP_WINDOW_SORT, T_MAP_BLOCK_DIR,
  T_MAP_PERMUTE_LDS, T_MAP_PERMUTE_GROUP, T_MAP_OWN_SORTS, T_MAP_CHILD_ROUNDS, T_CONV_SLAB_TRIM, T_CONV_ROW_TRIM,
  T_NEAREST_MAX_RING, T_INST_EVAL_FUSED, T_CONV_LEAN_EPI,
  T_COUNT
};
int64_t tune(Tune t);                                                   // current value (environment LGS_<NAME> at start, lgs_tuning_set later)
std::string dispatch_site_name(const char *kernel_text, const char *pretty_function);   // the name dispatch_site registers the site by
int dispatch_site(const char *kernel_text, const char *pretty_function);   // registers a launch site once -> its index
void dispatch_hit(int site);
// every kernel launch of the engine: counted per launch site (kernel expression + template bindings of the enclosing function)
#define LGS_KLAUNCH(kernel, ...)                                                                 \
  do {                                                                                           \
    static const int _lgs_site = lgs::dispatch_site(#kernel, __PRETTY_FUNCTION__);               \
    lgs::dispatch_hit(_lgs_site);                                                                \
    hipLaunchKernelGGL(kernel, __VA_ARGS__);                                                     \
  } while (0)

// a counter of its own among the launch sites (no kernel): `text` as it stands
#define LGS_COUNT(text)                                                                          \
  do {                                                                                           \
    static const int _lgs_site = lgs::dispatch_site(text, nullptr);                              \
    lgs::dispatch_hit(_lgs_site);                                                                \
  } while (0)

constexpr int kPadRows = 256;  // every position array is padded to a multiple of this
constexpr int kGroup = 64;     // rows per mask / tile_k entry (one wavefront of positions)

inline int64_t pad_rows(int64_t n) { return (n + kPadRows - 1) / kPadRows * kPadRows; }

// A view of a kernel map as an OUTPUT-STATIONARY gather table:
// position p in [0,n_pad) produces output row out_row[p] (or p itself) as
//     out[row(p)] = sum over slots s with nbr[s][p] >= 0 of  in[nbr[s][p]] . W[weight_index(s, p)]
struct View {
  const int32_t *nbr = nullptr;      // [KS][n_pad] input row per (slot, position), -1 = none; NULL = identity (1x1)
  const uint32_t *mask64 = nullptr;  // [n_pad/64] bit s set if any of the 64 positions has slot s   (KS > 1)
  const int32_t *tile_k = nullptr;   // [n_pad/64] weight index of the single slot, -1 = empty group (KS == 1, grouped)
  const int32_t *out_row = nullptr;  // [n_pad] output row per position, -1 = padding; NULL = identity
  int64_t n_pad = 0;
  int64_t n_out = 0;  // rows of the tensor this view writes
  int64_t n_in = 0;   // rows of the tensor it gathers from
  int KS = 1;         // slots per position (27 / 8 / 1)
  int K = 1;          // weight matrices of the op (27 / 8 / 1)
  int mirror = 0;     // weight index = K-1-s (the 3^3 map read in the dgrad direction)
  View() = default;
  View(int KS_, int K_, int64_t n_pad_, int64_t n_out_, int64_t n_in_) : n_pad(n_pad_), n_out(n_out_), n_in(n_in_), KS(KS_), K(K_) {}   // by its shape
};

// A segment map between a fine map and a coarser one (a stride-2^k descendant or the origin map):
// the fine rows of coarse row q are the fine SORTED positions [seg_start[q], seg_start[q+1]) -- one contiguous run, because
// coarsening masks low key bits and keeps the Morton sort, and the batch index is the top key field.
// Segments longer than kSegChunk rows are reduced in two passes over chunk items of at most kSegChunk rows each.
constexpr int kSegChunk = 512;
struct SegMap {
  const int32_t *fine_row = nullptr;    // [n_fine] sorted position -> fine row; NULL = identity (coarse levels)
  const int32_t *seg_start = nullptr;   // [n_coarse + 1]
  const int32_t *coarse_of = nullptr;   // [n_fine] coarse row of each fine sorted position
  const int32_t *item_start = nullptr;  // [n_coarse + 1] first chunk item of each segment (two-pass maps only)
  const int32_t *item_seg = nullptr;    // [n_items] segment of each chunk item, -1 = unused slot (two-pass maps only)
  const int32_t *row_seg = nullptr;     // [n_fine] coarse row of each fine ROW (origin segment maps only: the instance norm's apply)
  int64_t n_fine = 0, n_coarse = 0, n_items = 0;
  int64_t max_len = 0;                  // bound on the rows of one segment (8^k for stride 2^k); 0 = none (origin map)
  bool single_pass() const { return max_len > 0 && max_len <= kSegChunk; }
};

inline int pad32(int c) { return (c + 31) / 32 * 32; }
inline int esize(int dtype) { return dtype == LGS_BF16 ? 2 : 4; }
inline int epl(int dtype) { return dtype == LGS_BF16 ? 8 : 4; }

#if defined(__HIPCC__)
using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
typedef uint16_t bf16_t;  // storage type tag for bf16 tensors
__device__ inline float bf16_to_f32(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }
__device__ inline uint16_t f32_to_bf16(float f) {  // round to nearest even
  uint32_t u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__device__ inline float ld_elem(const float *p) { return *p; }
__device__ inline float ld_elem(const bf16_t *p) { return bf16_to_f32(*p); }
// pad rows [n, c] -> [n, cpad] (zero fill) for channel counts that are not a multiple of the load width (lgs_conv.hip, lgs_wgrad.hip)
template <typename T>
__global__ void k_pad_rows(const T *__restrict__ src, int64_t n, int c, int cpad, T *__restrict__ dst) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * cpad) return;
  int64_t r = i / cpad;
  int ch = (int)(i % cpad);
  dst[i] = ch < c ? src[r * c + ch] : (T)0;
}
// LDS-DMA kernels: the LDS destination of a buffer_load ... lds, and s_waitcnt vmcnt(n) with expcnt / lgkmcnt left alone (gfx9 encoding)
#define LGS_AS3(p) ((__attribute__((address_space(3))) void *)(p))
#define LGS_VMCNT(n) __builtin_amdgcn_s_waitcnt((((n) & 15) | (7 << 4) | (15 << 8) | (((n) >> 4) << 14)))
#endif

// lgs_wgrad.hip: everything a weight-gradient call decides on the host (kernel, tile, grid, workspace regions), see wgrad_plan()
using WgradPlan = lgs_wgrad_plan_info;
enum WgradPath { kWgEmpty = 0, kWgWide = 1, kWgPs = 2, kWgPairs = 3, kWgF32 = 4 };
int64_t wgrad_workspace_bytes(const lgs_kmap *km, int cin, int cout, int dtype);
// the next region of a workspace that is laid out front to back
inline lgs_conv_plan_region take_region(int64_t &used, int64_t bytes) {
  Layout l{used};
  const int64_t at = l.take(bytes);
  used = l.total();
  return {at, used - at};
}
// 1x1 stride-1 convolutions of the big maps as a streaming GEMM (lgs_pointwise.hip)
bool pointwise_supported(const View &v, int K, int g_real, int o_real, int64_t in_ld);
int launch_pointwise(const View &v, const void *in, int64_t in_ld, int g_real, const float *w, int cin_w, int cout_w, int transposed,
                     int o_real, const float *bias, void *out, hipStream_t s);
bool pointwise_f32_supported(const View &v, int K, int g_real, int o_real, int64_t in_ld);
int launch_pointwise_f32(const View &v, const void *in, int64_t in_ld, int g_real, const float *w, int cin_w, int cout_w, int transposed,
                         int o_real, const float *bias, void *out, hipStream_t s);
// lgs_conv_wide.hip: 2-D blocked forward / dgrad for >= 256 output channels (bf16); same packed weight image as k_conv_gather's wide tile
int launch_conv_wide(const View &v, const void *in, int cin_real, int in_ld, const void *wp, int nb_total, int ncp, int nbp, int K,
                     void *out, int cout_real, const float *bias, int gc64, hipStream_t s);
// lgs_wgrad_wide.hip: per-offset dense GEMM over compacted pair lists for >= 256 x 256 channel 3^3 weight gradients (bf16)
// (wgrad_wide_plan fills p and answers true where that kernel serves the call; in_ld = row stride of `in` in elements)
bool wgrad_wide_plan(const View &v, int cin, int cout, int in_ld, WgradPlan &p);
int launch_wgrad_wide(const View &v, const WgradPlan &p, const void *in, int cin, int in_ld, const void *gout, int cout, float *gw,
                      void *workspace, hipStream_t s);
// order `stream` after the construction of km's manager's maps (they are built on the manager's own stream)
int kmap_wait(lgs_kmap *km, hipStream_t stream);
int segmap_wait(lgs_segmap *sm, hipStream_t stream);

}  // namespace lgs

namespace lgs {
// ---- kernel-map relations.  What a request (in_key, out_key, kernel_size, dilation) names is decided ONCE, by classify_kmap; what
// follows from the answer is read from ONE table, traits_of.  Both map entry points, the plans, the conv entry points and the debug
// queries go through them (rows as in the contract of include/lgs_engine.h; tests/test_kmap_relation_cpu.py holds them to it).
enum KmapRelation {
  kRelIdentity = 0,      // kernel_size 1, in_key == out_key
  kRelConv3 = 1,         // kernel_size 3, in_key == out_key, dilation 1
  kRelConv2S2 = 2,       // kernel_size 2, out_key == stride2(in_key); the transposed conv walks the same object
  kRelConv3Dilated = 3,  // kernel_size 3, in_key == out_key, dilation >= 2
  kRelConv3S2 = 4,       // kernel_size 3, out_key == stride2(in_key)
  kRelConv1S2 = 5,       // kernel_size 1, out_key == stride2(in_key)
};
struct KmapTraits {
  int ks, K;
  bool strided;        // the out map is the in map's stride-2 map: the two views walk different row spaces
  bool bwd_mirror;     // bwd is the fwd table read from its other side (weight index K-1-s); else both views carry offset k in slot k
  bool transposed_ok;  // the conv entry points take `transposed` = 1 on it (the plain 3^3 stride-1 map refuses it as it always has)
  bool old_entry;      // lgs_manager_kernel_map builds it; the others are lgs_manager_kernel_map_ex's alone
  // k_wgrad_wide and k_wgrad_ps have been run and measured on the 3^3 stride-1 table and the 2^3 views only: a 3^3 map with two
  // different row spaces, and any 3^3 map walked by a transposed conv, goes to the pair-list / fp32 kernels, which take any view
  constexpr bool wgrad_pairs_only(bool transposed) const { return ks == 3 && (strided || transposed); }
};
constexpr KmapTraits traits_of(KmapRelation r) {
  switch (r) {           //                 ks   K  strided mirror transp  old
    case kRelConv3:        return KmapTraits{3, 27, false, true, false, true};
    case kRelConv2S2:      return KmapTraits{2, 8, true, false, true, true};
    case kRelConv3Dilated: return KmapTraits{3, 27, false, true, true, false};
    case kRelConv3S2:      return KmapTraits{3, 27, true, false, true, false};
    case kRelConv1S2:      return KmapTraits{1, 1, true, false, true, false};
    default:               return KmapTraits{1, 1, false, false, true, true};   // kRelIdentity
  }
}
constexpr int kCoordBits = 18;   // bits per coordinate in a packed key: every probed coordinate stays within 2^17 of a stored one
struct KmapRequest {
  bool ex;               // lgs_manager_kernel_map_ex asked (else lgs_manager_kernel_map, which has no dilation: taken as 1)
  bool same_key;         // in_key == out_key
  bool out_is_stride2;   // the out map was made by stride2(in_key)
  bool out_sorted;       // the out map's rows are in Morton order (order == nullptr)
  bool origin;           // either map is the origin map
  int ks, dilation, ts_in;
};
// -> nullptr and the relation, or the refusal (no HIP call; the checks in the order a caller of the entry point has always met them)
inline const char *classify_kmap(const KmapRequest &q, KmapRelation &rel) {
  if (q.origin) return q.ex ? "lgs_manager_kernel_map_ex: no kernel maps on the origin map" : "lgs_manager_kernel_map: no kernel maps on the origin map";
  const int d = q.ex ? q.dilation : 1;
  const bool strided = !q.same_key && q.out_is_stride2;
  if (d < 1) return "lgs_manager_kernel_map_ex: dilation must be >= 1";
  if (strided && d > 1) return "lgs_manager_kernel_map_ex: stride 2 combined with dilation > 1 is not supported";
  if (d > 1 && q.ks != 3) return "lgs_manager_kernel_map_ex: dilation > 1 needs kernel_size 3";
  if (d > 1) {
    if (!q.same_key) return "lgs_manager_kernel_map_ex: out_key must be in_key or stride2(in_key)";
    rel = kRelConv3Dilated;
  } else if (q.ks == 1 || q.ks == 3) {
    const char *refusal = q.ks == 1 ? "kernel_size 1 needs in_key == out_key" : "kernel_size 3 is supported for stride 1 (in_key == out_key) only";
    if (!q.same_key && !strided) return refusal;
    rel = q.ks == 1 ? (strided ? kRelConv1S2 : kRelIdentity) : (strided ? kRelConv3S2 : kRelConv3);
    if (!q.ex && !traits_of(rel).old_entry) return refusal;   // the old entry point refuses them as it always has
  } else if (q.ks == 2) {
    if (!strided) return "kernel_size 2 needs out_key == stride2(in_key)";
    rel = kRelConv2S2;
  } else {
    return "unsupported kernel_size (the model family uses 1, 2 and 3 only)";
  }
  if (!traits_of(rel).old_entry) {
    // the coarse-stationary views take "position == output row": a map made by stride2 has its rows in Morton order
    if (strided && !q.out_sorted) return "lgs_manager_kernel_map_ex: the stride-2 map's rows are not in sorted order";
    if ((int64_t)d * q.ts_in >= (1ll << (kCoordBits - 1))) return "lgs_manager_kernel_map_ex: dilation * tensor_stride must stay below 2^17";
  }
  return nullptr;
}
}  // namespace lgs

struct lgs_kmap {
  lgs_manager *mgr = nullptr;
  int in_key = -1, out_key = -1, ks = 1, K = 1;
  lgs::KmapRelation relation = lgs::kRelIdentity;   // with in_key, out_key and dilation: the cache key
  int dilation = 1;   // offset scale of a 3^3 stride-1 map in units of the tensor stride
  lgs::View fwd;  // gathers from the in map, writes the out map
  lgs::View bwd;  // gathers from the out map, writes the in map (dgrad / transposed conv)
};

namespace lgs {
inline KmapTraits traits_of(const lgs_kmap *km) { return traits_of(km->relation); }
// the relation of the synthetic map of a debug plan query, which carries the kernel size and two views by their row counts: two sides
// that differ in rows are a map and its stride-2 map (kernel size 2 names no other link); a dilated map plans as the plain 3^3 one
inline const char *synthetic_kmap_relation(lgs_kmap &km) {
  const bool same = km.ks != 2 && km.fwd.n_in == km.fwd.n_out;
  const char *refusal = classify_kmap(KmapRequest{true, same, !same, true, false, km.ks, 1, 1}, km.relation);
  if (!refusal) km.bwd.mirror = traits_of(km.relation).bwd_mirror ? 1 : 0;
  return refusal;
}
// the synthetic map itself, from the two views a debug plan query describes by plain integers: a table the view carries points at
// one word that no planner reads.  -> synthetic_kmap_relation's refusal, nullptr = a map of the family
inline const char *synthetic_kmap(const lgs_conv_plan_view &fwd, const lgs_conv_plan_view &bwd, int ks, lgs_kmap &km) {
  static const int32_t present = 0;
  auto view = [](const lgs_conv_plan_view &s) {
    View v;
    v.n_pad = s.n_pad; v.n_in = s.n_in; v.n_out = s.n_out; v.KS = s.KS; v.K = s.K;
    if (s.has_nbr) v.nbr = &present;
    if (s.has_nbr && s.KS > 1) v.mask64 = reinterpret_cast<const uint32_t *>(&present);
    if (s.has_tile_k) v.tile_k = &present;
    if (s.has_out_row) v.out_row = &present;
    return v;
  };
  km.ks = ks; km.K = fwd.K; km.fwd = view(fwd); km.bwd = view(bwd);
  return synthetic_kmap_relation(km);
}
}  // namespace lgs

struct lgs_segmap {
  lgs_manager *mgr = nullptr;
  int fine_key = -1, coarse_key = -1;
  lgs::SegMap sm;
};
