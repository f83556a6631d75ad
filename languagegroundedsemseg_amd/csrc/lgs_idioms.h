// lgs_idioms.h -- the small idioms the operator kernels share, each stated once: workspace layouts, binary searches, order-preserving
// keys, the rounded affine row, the open-addressed claim and the wave fold.  Sections 1 and 2 are plain C++ (tests/cpp/idioms_main.cpp
// includes this header alone and is built by the host compiler); section 3 exists under hipcc only.
#pragma once
#include <stdint.h>

#include "../../include/lgs_engine.h"   // constants only (plain C, no HIP)

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LGS_HD __host__ __device__ inline
#else
#define LGS_HD inline
#endif

namespace lgs {

// ---- 1. host arithmetic ---------------------------------------------------------------------------------------------------------
inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

// a workspace laid out front to back in 256-byte steps: take() answers the offset of the next region
struct Layout {
  int64_t used = 0;
  int64_t take(int64_t bytes) { const int64_t at = used; used += align256(bytes); return at; }
  int64_t total() const { return used; }
  template <typename T> static T *at(void *base, int64_t off) { return reinterpret_cast<T *>(static_cast<char *>(base) + off); }
};

// entries of an open-addressed table: `least` doubled until it holds `want` (the callers want twice their keys: at most half full)
inline int64_t table_pow2(int64_t least, int64_t want) {
  while (least < want) least <<= 1;
  return least;
}

// One layout function per operator: its *_workspace_bytes answers .total, its entry point carves with the offsets.  Every field is a
// byte offset in the order of the workspace; the sizes are what the entry points have always asked for, trailing slack included.

// lgs_ap.hip.  tmp_bytes = the larger temporary of rocPRIM's sort and scan
struct ApWs { int64_t tmp, keys, terms, skeys, rowstat, cnt, pfx, off, mn, total; };
inline ApWs ap_layout(int64_t n, int c, int64_t tmp_bytes) {
  Layout l;
  ApWs w;
  w.tmp = l.take(tmp_bytes);
  w.keys = w.terms = l.take(8 * (n + 1));   // the fp64 terms of stage 4 live where the unsorted keys did: those are dead after the sort
  w.skeys = l.take(8 * (n + 1));
  w.rowstat = l.take(8 * (n + 1));
  w.cnt = l.take(4 * (n + 1));
  w.pfx = l.take(4 * (n + 1));
  w.off = l.take(4 * (c + 1));
  w.mn = l.take(4 * (c + 1));
  l.take(256);                              // slack
  w.total = l.total();
  return w;
}

// lgs_cluster.hip.  tmp_bytes = rocPRIM's temporary of the pair sort; scal = [0] error flag, [1] cluster count
struct ClusterWs { int64_t tmp, keys, skeys, vals, svals, parent, size, scal, total; };
inline ClusterWs cluster_layout(int64_t n, int64_t tmp_bytes) {
  Layout l;
  const int64_t k = 8 * (n + 1), v = 4 * (n + 1);   // a column of keys, of int32 (a braced list is evaluated left to right)
  return {l.take(tmp_bytes), l.take(k), l.take(k), l.take(v), l.take(v), l.take(v), l.take(v), l.take(512), l.total()};
}

// lgs_insteval.hip: the id table of 2^k >= 2 g_cap entries, the slot counter, one partial maximum and sum per piece of a proposal.
// [0, zeroed) is cleared at the start of a call
constexpr int kInstChunk = 1024;   // members per workgroup of the overlap pass
inline uint32_t inst_table_size(int g_cap) { return (uint32_t)table_pow2(2, 2 * (int64_t)g_cap); }
inline int64_t inst_pieces(int64_t m, int p) { return (m + kInstChunk - 1) / kInstChunk + p + 1; }
struct InstOverlapWs { int64_t t_key, t_cnt, n_slots, zeroed, part_max, part_sum, total; };
inline InstOverlapWs inst_overlap_layout(int64_t m, int p, int g_cap) {
  Layout l;
  InstOverlapWs w;
  const int64_t t = inst_table_size(g_cap);
  w.t_key = l.take(8 * t);
  w.t_cnt = l.take(4 * t);
  w.n_slots = l.take(256);
  w.zeroed = l.total();
  w.part_max = l.take(4 * inst_pieces(m, p));
  w.part_sum = l.take(8 * inst_pieces(m, p));
  w.total = l.total();
  return w;
}

// lgs_insttarget.hip: the instance table of 2^k >= 2 inst_cap entries (key, point count, three coordinate sums, min, max: filled per
// entry, moved to the entry's output row once the rows are known) and the row of every entry
constexpr int kInstTargetMaxCap = 65536;
inline uint32_t inst_target_table_size(int inst_cap) { return (uint32_t)table_pow2(64, 2 * (int64_t)inst_cap); }
struct InstTargetWs { int64_t t_key, t_cnt, t_sum, t_min, t_max, t_row, total; };
inline InstTargetWs inst_target_layout(int inst_cap) {
  Layout l;
  const int64_t t = inst_target_table_size(inst_cap);
  return {l.take(8 * t), l.take(4 * t), l.take(24 * t), l.take(12 * t), l.take(12 * t), l.take(4 * t), l.total()};
}

// lgs_augment.hip, elastic distortion: one slot of max_cells x 3 floats per scene, noise then field
struct ElasticWs { int64_t noise, field, total; };
inline ElasticWs elastic_layout(int b, int64_t max_cells) {
  Layout l;
  const int64_t slots = (int64_t)b * max_cells * 3 * (int64_t)sizeof(float);
  return {l.take(slots), l.take(slots), l.total()};
}

// lgs_paste.hip.  cap = entries of the instance-voxel table: a power of two, at least twice the instance rows
constexpr int kPasteStatsBytes = 64;   // sizeof(SlotStats)
struct PasteWs {
  int64_t off, bounds, flags, stats, place, hkeys, hmin, hslot, ivox, maps, total;
  int64_t cap;
};
inline int64_t table_cap(int64_t inst_rows) { return table_pow2(64, 2 * inst_rows); }
inline PasteWs paste_layout(int b, int slots, int64_t inst_rows, int64_t max_map_cells) {
  Layout l;
  PasteWs w;
  const int64_t slots1 = slots > 1 ? slots : 1, rows1 = inst_rows > 1 ? inst_rows : 1;
  w.cap = table_cap(inst_rows);
  w.off = l.take((int64_t)sizeof(int64_t) * (b + 1));
  w.bounds = l.take((int64_t)sizeof(int32_t) * 6 * b);
  w.flags = l.take((int64_t)sizeof(int32_t) * LGS_AUG_MAX_SCENES);
  w.stats = l.take(kPasteStatsBytes * slots1);
  w.place = l.take((int64_t)sizeof(int32_t) * 4 * slots1);
  w.hkeys = l.take((int64_t)sizeof(uint64_t) * w.cap);
  w.hmin = l.take((int64_t)sizeof(int32_t) * w.cap);
  w.hslot = l.take((int64_t)sizeof(int32_t) * rows1);
  w.ivox = l.take((int64_t)sizeof(int32_t) * 4 * rows1);
  w.maps = l.take((int64_t)sizeof(int32_t) * b * max_map_cells);
  w.total = l.total();
  return w;
}

// lgs_dropout.hip: one record per scene, one table of 2048 64-bit bins per (digit, scene), and two words per tile.  A tile is
// kDropTile rows of one scene, so n rows in b scenes make at most n / kDropTile + b of them
constexpr int kDropTile = 2048;
constexpr int kDropSceneBytes = 24;    // sizeof(DropScene)
constexpr int64_t kDropMaxRows = 1ll << 40;
struct DropoutWs { int64_t scenes, hist, tile_lt, tile_eq, total, tiles; };
inline DropoutWs dropout_layout(int64_t n, int b) {
  Layout l;
  DropoutWs w;
  w.tiles = n / kDropTile + b;
  w.scenes = l.take((int64_t)kDropSceneBytes * b);
  w.hist = l.take((int64_t)sizeof(uint64_t) * 3 * b * 2048);
  w.tile_lt = l.take((int64_t)sizeof(int64_t) * w.tiles);
  w.tile_eq = l.take((int64_t)sizeof(int64_t) * w.tiles);
  w.total = l.total();
  return w;
}

// lgs_instshift.hip: rocPRIM's temporary of the row sort, the segment table of 2^k >= 2 seg_cap entries (key, row count, three minima
// and three maxima as order-preserving keys, the entry's rank), one record per segment in rank order, two flag words, and per row the
// segment (entry, then rank), the sort key, the sorted key and the sorted row
constexpr int kInstShiftMaxCap = 65536;
constexpr int kInstShiftMaxTail = 256;
constexpr int kInstShiftSegBytes = 24;   // sizeof(ShiftSeg)
inline uint32_t inst_shift_table_size(int seg_cap) { return (uint32_t)table_pow2(64, 2 * (int64_t)seg_cap); }
struct InstShiftWs { int64_t tmp, t_key, t_cnt, t_lo, t_hi, t_row, segs, flags, slot, keys, skeys, srows, total; };
inline InstShiftWs inst_shift_layout(int64_t n, int seg_cap, int64_t tmp_bytes) {
  Layout l;
  const int64_t t = inst_shift_table_size(seg_cap), v = 4 * (n + 1);
  return {l.take(tmp_bytes), l.take(8 * t), l.take(4 * t), l.take(12 * t), l.take(12 * t), l.take(4 * t),
          l.take((int64_t)kInstShiftSegBytes * seg_cap), l.take(256), l.take(v), l.take(v), l.take(v), l.take(v), l.total()};
}

// lgs_fps.hip: one record per segment, and one (x, y, z, t) record per position for the segments that keep their state in memory
constexpr int kFpsSegBytes = 24;         // sizeof(FpsSeg)
constexpr int64_t kFpsMaxRows = (1ll << 31) - 2;
constexpr int64_t kFpsMaxSegments = 1ll << 20;
struct FpsWs { int64_t segs, state, total; };
inline FpsWs fps_layout(int64_t n, int64_t s) {
  Layout l;
  return {l.take((int64_t)kFpsSegBytes * (s + 1)), l.take(16 * (n + 1)), l.total()};
}

// ---- 2. pure functions ----------------------------------------------------------------------------------------------------------
// Binary searches over p[lo, hi), non-decreasing.  I is the index type of the caller (int or int64_t).
// the first index whose element is not below k (hi if there is none)
template <typename T, typename I, typename K>
LGS_HD I lower_bound(const T *p, I lo, I hi, K k) {
  while (lo < hi) {
    const I mid = (lo + hi) >> 1;
    if (p[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the first index whose element is above x (hi if there is none)
template <typename T, typename I, typename X>
LGS_HD I upper_bound(const T *p, I lo, I hi, X x) {
  while (lo < hi) {
    const I mid = (lo + hi) >> 1;
    if (p[mid] > x) hi = mid; else lo = mid + 1;
  }
  return lo;
}
// the last record t in [0, count) with p[stride t] <= i, for a table of `count` records of `stride` elements whose starts p[stride t]
// do not decrease: the record that row i lies in.  An empty record shares its start with the next one and loses to it.  0 if every
// start is above i, or the table is empty.
template <typename T>
LGS_HD int last_not_above(const T *p, int stride, int count, T i) {
  int lo = 0, hi = count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p[stride * mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Order-preserving 32-bit keys, for integer atomicMin / atomicMax and for sorting: a < b <=> key(a) < key(b).  The float map is the
// plain one: -0.0 < +0.0, NaNs lie beyond the infinities by their sign.  A caller that wants another rule for those values applies it
// in front (lgs_ap.hip: -0 counts as +0; lgs_insteval.hip: any NaN is the top key).
LGS_HD uint32_t ord_key_of_bits(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }   // u = the float's bit pattern
LGS_HD uint32_t ord_key(float f) { return ord_key_of_bits(__builtin_bit_cast(uint32_t, f)); }
LGS_HD float ord_key_inv(uint32_t k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
LGS_HD uint32_t ikey(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
LGS_HD int32_t ikey_inv(uint32_t k) { return (int32_t)(k ^ 0x80000000u); }

// ---- 3. device only -------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
// one row of an affine [3, 4] applied to (x, y, z, 1) in double: ((x a0 + y a1) + z a2) + a3, every operation rounded, no contraction.
// The voxeliser, its batched form, the paste and the nearest-site query all call this one, so floor() sees the same bits in each.
__device__ inline double affine_row(const double *a, double x, double y, double z) {
  return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(x, a[0]), __dmul_rn(y, a[1])), __dmul_rn(z, a[2])), a[3]);
}

// Open addressing with linear probes: the slot s = start, start + 1, ... (mod mask + 1) of keys[] that this call claimed for `key` by
// compare-and-swap against `empty`, or that already held `key`; -1 after max_probes slots that hold other keys (a full table).
// K is a 32- or 64-bit integer type atomicCAS takes; keys may be global or LDS memory.  The hash and the start slot are the caller's.
template <typename K>
__device__ inline int64_t table_claim(K *keys, uint64_t start, uint64_t mask, K key, K empty, uint64_t max_probes) {
  uint64_t s = start;
#pragma unroll 1
  for (uint64_t probe = 0; probe < max_probes; ++probe) {
    const K prev = atomicCAS(keys + s, empty, key);
    if (prev == empty || prev == key) return (int64_t)s;
    s = (s + 1) & mask;
  }
  return -1;
}

// The xor butterfly WIDTH / 2 .. 1 over groups of WIDTH lanes: every lane ends with the fold of its group.  The order is part of the
// contract: floating-point folds give the same bits in every lane and in every call.
template <int WIDTH = 64, typename T, typename Op>
__device__ inline T wave_fold(T v, Op op) {
#pragma unroll
  for (int o = WIDTH / 2; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, WIDTH));
  return v;
}
template <int WIDTH = 64, typename T> __device__ inline T wave_sum(T v) { return wave_fold<WIDTH>(v, [](T a, T b) { return a + b; }); }
template <int WIDTH = 64, typename T> __device__ inline T wave_min(T v) { return wave_fold<WIDTH>(v, [](T a, T b) { return b < a ? b : a; }); }
template <int WIDTH = 64, typename T> __device__ inline T wave_max(T v) { return wave_fold<WIDTH>(v, [](T a, T b) { return b > a ? b : a; }); }
#endif

}  // namespace lgs
