// lgs_instshift.hip -- the reference's per-instance colour and scale shifts (instance_augmentation == 'raw') on the device, gfx950.
//
// Replaces ScannetVoxelizationDataset.augment_instances (lib/datasets/scannet.py:243-319: per tail instance one boolean mask over the
// whole cloud, then np.delete / np.vstack of the cloud) with InstanceAugmentation (lib/transforms.py:288-382).
// A SEGMENT is the set of rows of one scene that share (label in the tail list, instance id).  Its key is
// ((scene * 256 + index of the label in the sorted tail list) << 32) | id, so key order is the reference's loop order; all ones names no key.
// Launches of one call, in stream order, nothing read back:
//   k_is_init     the segment table is emptied.
//   k_is_fold     a workgroup combines its 2048 rows in an LDS table of 512 entries (count, three minima and three maxima as
//                 order-preserving keys: LDS integer atomics) and adds every distinct segment ONCE to its entry of the global table
//                 (open addressing, table_claim).  A key that finds no LDS entry in 8 probes goes to the global table directly.  The
//                 row remembers its global entry in slot[].  Membership of the tail list is a binary search in LDS.
//   k_is_decide   an entry's rank is the number of keys in the table below its own (the walk of k_it_rows); the segment's decision
//                 (one Philox block, or the forced table), fl32(f), fl32(1 - f) and the centre go to record `rank`.
//   k_is_keys     per row the sort key scene * (seg_cap + 1) + (0 for a row of no segment, 1 + rank otherwise); slot[] goes from
//                 entry to rank.
//   rocPRIM       one stable radix sort of (key, row) over the bits the keys use: rows of no segment first, ascending, then the
//                 segments in key order, rows ascending -- the reference's np.delete + np.vstack order, scene by scene.
//   k_is_apply    one streaming pass: output row j reads source row order[j], scaled / recoloured by its segment's record.
// Every cross-workgroup combination is an integer atomic (add, min, max, or), the ranks do not depend on which entry a key claimed,
// and the sort is stable: the result does not depend on any launch grid and two calls give the same bits.
// More than seg_cap segments: a scene that holds a segment of rank >= seg_cap is left as it is (identity order, attribute 0), bit
// `scene` of status[0]; more distinct segments than the table has entries (>= 2 seg_cap): every scene is.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "lgs_common.h"
#include "lgs_philox.h"

namespace lgs {

namespace {

constexpr int kScenes = LGS_AUG_MAX_SCENES;
constexpr int kThreads = 256;
constexpr int kPerThread = 8;
constexpr int kFoldRows = kThreads * kPerThread;     // rows per workgroup of the fold pass
constexpr int kLds = 512;                            // entries of its LDS table
constexpr int kLdsProbes = 8;
constexpr int kRankTile = 2048;
constexpr unsigned long long kEmpty = ~0ull;
constexpr uint32_t kKeyPosInf = 0xFF800000u;         // ord_key(+inf)
constexpr uint32_t kKeyNegInf = 0x007FFFFFu;         // ord_key(-inf)

struct TailList { int64_t v[kInstShiftMaxTail]; int n; };
struct SceneSeeds { uint32_t v[kScenes]; };
struct ShiftSeg {            // one per segment, in rank order
  float f, g, c[3];          // fl32(f), fl32(1 - f), the centre ((lo_x + hi_x) / 2, (lo_y + hi_y) / 2, lo_z)
  int32_t attr;              // 0 nothing, 1 .. 6 colour (Red, Green, Blue, Yellow, Dark, Bright), 7 scale up, 8 scale down
};
static_assert(sizeof(ShiftSeg) == kInstShiftSegBytes, "inst_shift_layout sizes the segment records");
struct Flags { uint32_t bad, full; };                // scenes with a segment of rank >= seg_cap; the table overflowed

__device__ inline uint32_t hash_key(unsigned long long h) {
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  return (uint32_t)h;
}

// the offsets, clamped into a non-decreasing table on [0, n] -> LDS (every workgroup that needs a row's scene does this)
__device__ inline void load_offsets(const int64_t *__restrict__ scene_offsets, int64_t n, int b, int64_t (&off)[kScenes + 1]) {
  if ((int)threadIdx.x <= b) off[threadIdx.x] = threadIdx.x == 0 ? 0 : (int)threadIdx.x == b ? n : scene_offsets[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t prev = 0;
    for (int s = 1; s <= b; ++s) prev = off[s] = std::min(std::max(off[s], prev), n);
  }
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void k_is_init(unsigned long long *__restrict__ t_key, int32_t *__restrict__ t_cnt,
                                                      uint32_t *__restrict__ t_lo, uint32_t *__restrict__ t_hi, uint32_t tsize,
                                                      Flags *__restrict__ flags) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j == 0) *flags = Flags{0u, 0u};
  if (j >= tsize) return;
  t_key[j] = kEmpty;
  t_cnt[j] = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    t_lo[3 * (int64_t)j + a] = 0xFFFFFFFFu;
    t_hi[3 * (int64_t)j + a] = 0u;
  }
}

__device__ inline void global_merge(int32_t *__restrict__ t_cnt, uint32_t *__restrict__ t_lo, uint32_t *__restrict__ t_hi, int64_t e, int c,
                                    const uint32_t *lo, const uint32_t *hi) {
  atomicAdd(&t_cnt[e], c);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    atomicMin(&t_lo[3 * e + a], lo[a]);
    atomicMax(&t_hi[3 * e + a], hi[a]);
  }
}

__global__ __launch_bounds__(kThreads) void k_is_fold(const float *__restrict__ points, const int64_t *__restrict__ labels,
                                                      const int64_t *__restrict__ ids, int64_t n, const int64_t *__restrict__ scene_offsets,
                                                      int b, TailList tail, unsigned long long *__restrict__ t_key,
                                                      int32_t *__restrict__ t_cnt, uint32_t *__restrict__ t_lo, uint32_t *__restrict__ t_hi,
                                                      uint32_t tmask, int32_t *__restrict__ slot, Flags *__restrict__ flags,
                                                      int32_t *__restrict__ status) {
  __shared__ unsigned long long l_key[kLds];
  __shared__ uint32_t l_lo[kLds * 3], l_hi[kLds * 3];
  __shared__ int32_t l_cnt[kLds], l_entry[kLds];
  __shared__ int64_t l_tail[kInstShiftMaxTail];
  __shared__ int64_t l_off[kScenes + 1];
  load_offsets(scene_offsets, n, b, l_off);
  for (int j = threadIdx.x; j < kLds; j += kThreads) {
    l_key[j] = kEmpty;
    l_cnt[j] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      l_lo[3 * j + a] = 0xFFFFFFFFu;
      l_hi[3 * j + a] = 0u;
    }
  }
  if ((int)threadIdx.x < tail.n) l_tail[threadIdx.x] = tail.v[threadIdx.x];
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * kFoldRows;
  int mine[kPerThread];                    // the LDS entry of my k-th row; -1: the row is done (no segment, or sent directly)
  uint32_t bad_id = 0u;
  bool full = false;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int64_t i = i0 + (int64_t)k * kThreads + threadIdx.x;
    mine[k] = -1;
    if (i >= n) continue;
    const int64_t lab = labels[i];
    const int q = lower_bound(l_tail, 0, tail.n, lab);
    if (q >= tail.n || l_tail[q] != lab) { slot[i] = -1; continue; }
    const int64_t id = ids[i];
    const int s = last_not_above(l_off, 1, b, i);
    if (id < 0 || id >= (1ll << 31)) {
      if (id != -1) bad_id |= 1u << s;
      slot[i] = -1;
      continue;
    }
    const unsigned long long key = ((unsigned long long)(uint32_t)(s * kInstShiftMaxTail + q) << 32) | (unsigned long long)id;
    const uint32_t hk = hash_key(key);
    uint32_t p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = ord_key(points[3 * i + a]);
    uint32_t h = hk & (kLds - 1);
#pragma unroll 1
    for (int probe = 0; probe < kLdsProbes; ++probe) {
      const unsigned long long prev = atomicCAS(&l_key[h], kEmpty, key);
      if (prev == kEmpty || prev == key) { mine[k] = (int)h; break; }
      h = (h + 1) & (kLds - 1);
    }
    if (mine[k] >= 0) {
      const int e = mine[k];
      atomicAdd(&l_cnt[e], 1);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        // the entry only ever moves towards the extreme, so a value that does not improve on what it shows now never will
        if (p[a] < *(volatile uint32_t *)&l_lo[3 * e + a]) atomicMin(&l_lo[3 * e + a], p[a]);
        if (p[a] > *(volatile uint32_t *)&l_hi[3 * e + a]) atomicMax(&l_hi[3 * e + a], p[a]);
      }
    } else {
      const int64_t g = table_claim(t_key, hk & tmask, tmask, key, kEmpty, (uint64_t)tmask + 1);
      if (g >= 0) global_merge(t_cnt, t_lo, t_hi, g, 1, p, p);
      else full = true;
      slot[i] = (int32_t)g;
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < kLds; j += kThreads) {
    const unsigned long long key = l_key[j];
    if (key == kEmpty) continue;
    const int64_t g = table_claim(t_key, hash_key(key) & tmask, tmask, key, kEmpty, (uint64_t)tmask + 1);
    l_entry[j] = (int32_t)g;
    if (g >= 0) global_merge(t_cnt, t_lo, t_hi, g, l_cnt[j], &l_lo[3 * j], &l_hi[3 * j]);
    else full = true;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int64_t i = i0 + (int64_t)k * kThreads + threadIdx.x;
    if (mine[k] >= 0) slot[i] = l_entry[mine[k]];
  }
  if (bad_id) atomicOr(status + 1, (int32_t)bad_id);
  if (full) atomicOr(&flags->full, 1u);
}

struct Forced {              // the teacher-forced decisions: keys [m, 3] = (scene, label, id); keys == NULL: the generator draws
  const int64_t *keys;
  const int32_t *attr;
  const double *factor;
  int m;
};

// one segment's decision -> (attribute, factor).  ext: the segment's extents, scene: the scene's (fp32, hi - lo)
__device__ inline int decide(int s, int64_t label, uint32_t id, const float (&ext)[3], const float (&scene)[3], const Forced &forced,
                             double p_color, double p_scale, uint32_t seed_lo, uint32_t seed_hi, uint32_t scene_seed, double &f) {
  f = 1.0;
  if (forced.keys) {
    for (int j = 0; j < forced.m; ++j)
      if (forced.keys[3 * j] == s && forced.keys[3 * j + 1] == label && forced.keys[3 * j + 2] == (int64_t)id) {
        f = forced.factor[j];
        return forced.attr[j];
      }
    return 0;
  }
  uint32_t c[4] = {id, (uint32_t)label, (uint32_t)((uint64_t)label >> 32), (uint32_t)LGS_AUG_STAGE_INSTSHIFT ^ seed_hi};
  philox4x32_10(c, seed_lo, scene_seed);
  const double r = 1.0 / 4294967296.0;
  const double u0 = (double)c[0] * r, u1 = (double)c[1] * r, u2 = (double)c[2] * r, u3 = (double)c[3] * r;      // exact
  if (u0 < p_color) return 1 + (int)(6.0 * u2);
  if (!(u1 < p_scale)) return 0;
  if (!(2.0 * u2 > 1.0)) {
    f = __dadd_rn(0.5, __dmul_rn(0.5, u3));
    return 8;
  }
  double h = 1.5;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float q = __fdiv_rn(scene[a], ext[a]);
    if (isfinite(q)) h = fmin(h, (double)q);
  }
  f = __dadd_rn(1.0, __dmul_rn(__dsub_rn(h, 1.0), u3));
  return 7;
}

// an occupied entry's rank is the number of keys in the table below its own (the empty key is above all); its record goes there
__global__ __launch_bounds__(kThreads) void k_is_decide(const unsigned long long *__restrict__ t_key, const uint32_t *__restrict__ t_lo,
                                                        const uint32_t *__restrict__ t_hi, uint32_t tsize, int seg_cap,
                                                        const float *__restrict__ scene_bounds, TailList tail, Forced forced,
                                                        double p_color, double p_scale, uint32_t seed_lo, uint32_t seed_hi,
                                                        SceneSeeds seeds, int32_t *__restrict__ t_row, ShiftSeg *__restrict__ segs,
                                                        Flags *__restrict__ flags) {
  __shared__ unsigned long long l_tile[kRankTile];
  __shared__ uint32_t l_m;
  const uint32_t h = blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long k = h < tsize ? t_key[h] : kEmpty;
  if (h < tsize) t_row[h] = -1;
  if (!__syncthreads_or(k != kEmpty)) return;
  uint32_t r = 0;
  for (uint32_t base = 0; base < tsize; base += kRankTile) {
    // the occupied keys of this tile of the table, packed (in any order: they are only counted)
    const uint32_t end = tsize - base < (uint32_t)kRankTile ? tsize : base + (uint32_t)kRankTile;
    __syncthreads();
    if (threadIdx.x == 0) l_m = 0;
    __syncthreads();
    unsigned long long other[kRankTile / kThreads];
#pragma unroll
    for (int q = 0; q < kRankTile / kThreads; ++q) {
      const uint32_t j = base + q * kThreads + threadIdx.x;
      other[q] = j < end ? t_key[j] : kEmpty;
    }
#pragma unroll
    for (int q = 0; q < kRankTile / kThreads; ++q)
      if (other[q] != kEmpty) l_tile[atomicAdd(&l_m, 1u)] = other[q];
    __syncthreads();
    const uint32_t m = l_m;                  // <= kRankTile
    if (k != kEmpty) {
#pragma unroll 4
      for (uint32_t j = 0; j < m; ++j) r += l_tile[j] < k ? 1u : 0u;
    }
  }
  if (k == kEmpty) return;
  const int s = (int)(k >> 40), q = (int)((k >> 32) & (kInstShiftMaxTail - 1));
  if (r >= (uint32_t)seg_cap) {
    atomicOr(&flags->bad, 1u << s);
    return;
  }
  float lo[3], ext[3], scene[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = ord_key_inv(t_lo[3 * (int64_t)h + a]);
    ext[a] = __fsub_rn(ord_key_inv(t_hi[3 * (int64_t)h + a]), lo[a]);
    scene[a] = __fsub_rn(scene_bounds[6 * s + 3 + a], scene_bounds[6 * s + a]);
  }
  double f;
  ShiftSeg seg;
  seg.attr = decide(s, tail.v[q], (uint32_t)k, ext, scene, forced, p_color, p_scale, seed_lo, seed_hi, seeds.v[s], f);
  if (seg.attr < 0 || seg.attr > 8) seg.attr = 0;
  seg.f = (float)f;
  seg.g = (float)__dsub_rn(1.0, f);
  seg.c[0] = __fmul_rn(__fadd_rn(lo[0], ord_key_inv(t_hi[3 * (int64_t)h + 0])), 0.5f);
  seg.c[1] = __fmul_rn(__fadd_rn(lo[1], ord_key_inv(t_hi[3 * (int64_t)h + 1])), 0.5f);
  seg.c[2] = lo[2];
  segs[r] = seg;
  t_row[h] = (int32_t)r;
}

// scenes that stay as they are
__device__ inline uint32_t bad_scenes(const Flags *__restrict__ flags) { return flags->full ? 0xFFFFFFFFu : flags->bad; }

__global__ __launch_bounds__(kThreads) void k_is_keys(int64_t n, const int64_t *__restrict__ scene_offsets, int b, int seg_cap,
                                                      const int32_t *__restrict__ t_row, const Flags *__restrict__ flags,
                                                      int32_t *__restrict__ slot, uint32_t *__restrict__ keys, int32_t *__restrict__ status) {
  __shared__ int64_t l_off[kScenes + 1];
  load_offsets(scene_offsets, n, b, l_off);
  const uint32_t bad = bad_scenes(flags);
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i == 0 && bad) atomicOr(status, (int32_t)(b == kScenes ? bad : bad & ((1u << b) - 1u)));
  if (i >= n) return;
  const int s = last_not_above(l_off, 1, b, i);
  const int32_t h = slot[i];
  const int32_t r = (h >= 0 && !((bad >> s) & 1u)) ? t_row[h] : -1;
  slot[i] = r;
  keys[i] = (uint32_t)s * (uint32_t)(seg_cap + 1) + (uint32_t)(r + 1);
}

__global__ __launch_bounds__(kThreads) void k_is_apply(const float *__restrict__ points, const float *__restrict__ colors,
                                                       const int64_t *__restrict__ labels, const int64_t *__restrict__ ids, int64_t n,
                                                       const uint32_t *__restrict__ srows, const int32_t *__restrict__ slot,
                                                       const ShiftSeg *__restrict__ segs, int hue_as_written, float *__restrict__ points_out,
                                                       float *__restrict__ colors_out, int64_t *__restrict__ labels_out,
                                                       int64_t *__restrict__ ids_out, int64_t *__restrict__ order) {
  const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  const int64_t i = srows[j];
  const int32_t r = slot[i];
  float p[3], c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    p[a] = points[3 * i + a];
    c[a] = colors[3 * i + a];
  }
  int attr = 0;
  if (r >= 0) {
    const ShiftSeg seg = segs[r];
    attr = seg.attr;
    if (attr >= 7) {
#pragma unroll
      for (int a = 0; a < 3; ++a) p[a] = __fadd_rn(__fmul_rn(p[a], seg.f), __fmul_rn(seg.c[a], seg.g));
    } else if (attr == 5) {
#pragma unroll
      for (int a = 0; a < 3; ++a) c[a] = truncf(__fmul_rn(c[a], 0.5f));
    } else if (attr == 6) {
#pragma unroll
      for (int a = 0; a < 3; ++a) c[a] = truncf(__fsub_rn(255.f, __fdiv_rn(__fsub_rn(255.f, c[a]), 2.f)));
    } else if (attr >= 1) {
      // Red {r}, Green {g}, Blue {b}, Yellow {r, g}.  As written, the reference's hsv_to_rgb rounds [0, 1] values to uint8 before the
      // * 255: a channel is 255 iff the row's maximum is 255 and the channel is in the hue's set or the row is grey, else 0
      const float mx = fmaxf(fmaxf(c[0], c[1]), c[2]), mn = fminf(fminf(c[0], c[1]), c[2]);
      const bool in_set[3] = {attr == 1 || attr == 4, attr == 2 || attr == 4, attr == 3};
#pragma unroll
      for (int a = 0; a < 3; ++a)
        c[a] = hue_as_written ? ((mx == 255.f && (in_set[a] || mx == mn)) ? 255.f : 0.f) : (in_set[a] ? mx : mn);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    points_out[3 * j + a] = p[a];
    colors_out[3 * j + a] = c[a];
  }
  labels_out[2 * j] = labels[i];
  labels_out[2 * j + 1] = attr;
  ids_out[j] = ids[i];
  order[j] = i;
}

inline bool shift_shape_ok(int64_t n, int b, int seg_cap) {
  return n >= 0 && n < (1ll << 31) - 1 && b >= 1 && b <= kScenes && seg_cap >= 1 && seg_cap <= kInstShiftMaxCap;
}

// bits of the largest sort key, (b - 1) (seg_cap + 1) + seg_cap
inline unsigned key_bits(int b, int seg_cap) {
  unsigned bits = 1;
  while (((int64_t)b * (seg_cap + 1) - 1) >> bits) ++bits;
  return bits;
}

// the one sort: (key, row) by key over [0, bits), stable, the rows counted on the fly.  tmp == NULL: the size query (no launch)
inline hipError_t sort_rows(void *tmp, size_t &tmp_bytes, const uint32_t *keys, uint32_t *skeys, uint32_t *srows, int64_t n, unsigned bits,
                            hipStream_t s) {
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, skeys, rocprim::counting_iterator<uint32_t>(0u), srows, (size_t)(n > 0 ? n : 1),
                                   0u, bits, s);
}

}  // namespace

}  // namespace lgs

using namespace lgs;

extern "C" {

int64_t lgs_instance_shift_workspace_bytes(int64_t n, int b, int seg_cap) {
  if (!shift_shape_ok(n, b, seg_cap)) return 0;
  size_t tb = 0;
  if (sort_rows(nullptr, tb, nullptr, nullptr, nullptr, n, key_bits(b, seg_cap), (hipStream_t)0) != hipSuccess) return 0;
  return inst_shift_layout(n, seg_cap, (int64_t)tb).total;
}

int lgs_instance_shift(const float *points, const float *colors, const int64_t *labels, const int64_t *instance_ids, int64_t n,
                       const int64_t *scene_offsets, int b, const float *scene_bounds, const int64_t *tail_labels, int n_tail,
                       double color_prob, double scale_prob, int64_t seed, const int32_t *scene_seeds, const int64_t *forced_keys,
                       const int32_t *forced_attr, const double *forced_factor, int n_forced, int hue_as_written, int seg_cap,
                       void *workspace, float *points_out, float *colors_out, int64_t *labels_out, int64_t *instances_out,
                       int64_t *order, int32_t *status, void *stream) {
  LGS_REQUIRE(b >= 1 && b <= kScenes, "lgs_instance_shift: 1 <= b <= LGS_AUG_MAX_SCENES");
  LGS_REQUIRE(seg_cap >= 1 && seg_cap <= kInstShiftMaxCap, "lgs_instance_shift: seg_cap must be in 1 .. 65536");
  LGS_REQUIRE(n_tail >= 0 && n_tail <= kInstShiftMaxTail && (n_tail == 0 || tail_labels), "lgs_instance_shift: at most 256 tail labels");
  LGS_REQUIRE(color_prob >= 0.0 && color_prob <= 1.0 && scale_prob >= 0.0 && scale_prob <= 1.0,
              "lgs_instance_shift: the probabilities must lie in [0, 1]");
  LGS_REQUIRE(n_forced >= 0 && (n_forced == 0 || (forced_keys && forced_attr && forced_factor)) && (forced_keys || (!forced_attr && !forced_factor)),
              "lgs_instance_shift: the forced table needs keys, attributes and factors");
  LGS_REQUIRE(shift_shape_ok(n, b, seg_cap) && scene_offsets && scene_bounds && workspace && status, "lgs_instance_shift: bad argument");
  LGS_REQUIRE(n == 0 || (points && colors && labels && instance_ids && points_out && colors_out && labels_out && instances_out && order),
              "lgs_instance_shift: null row argument");
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const unsigned bits = key_bits(b, seg_cap);
  size_t tb = 0;
  LGS_HIP(sort_rows(nullptr, tb, nullptr, nullptr, nullptr, n, bits, s));
  const InstShiftWs w = inst_shift_layout(n, seg_cap, (int64_t)tb);
  const uint32_t tsize = inst_shift_table_size(seg_cap);
  unsigned long long *t_key = Layout::at<unsigned long long>(workspace, w.t_key);
  int32_t *t_cnt = Layout::at<int32_t>(workspace, w.t_cnt), *t_row = Layout::at<int32_t>(workspace, w.t_row);
  uint32_t *t_lo = Layout::at<uint32_t>(workspace, w.t_lo), *t_hi = Layout::at<uint32_t>(workspace, w.t_hi);
  ShiftSeg *segs = Layout::at<ShiftSeg>(workspace, w.segs);
  Flags *flags = Layout::at<Flags>(workspace, w.flags);
  int32_t *slot = Layout::at<int32_t>(workspace, w.slot);
  uint32_t *keys = Layout::at<uint32_t>(workspace, w.keys), *skeys = Layout::at<uint32_t>(workspace, w.skeys);
  uint32_t *srows = Layout::at<uint32_t>(workspace, w.srows);
  TailList tail;
  std::memset(&tail, 0, sizeof(tail));
  std::copy(tail_labels, tail_labels + n_tail, tail.v);
  std::sort(tail.v, tail.v + n_tail);
  tail.n = (int)(std::unique(tail.v, tail.v + n_tail) - tail.v);
  SceneSeeds seeds;
  for (int i = 0; i < kScenes; ++i) seeds.v[i] = (scene_seeds && i < b) ? (uint32_t)scene_seeds[i] : 0u;
  const Forced forced{forced_keys, forced_attr, forced_factor, n_forced};
  const unsigned tblocks = (tsize + kThreads - 1) / kThreads, rblocks = (unsigned)((n + kThreads - 1) / kThreads);
  LGS_KLAUNCH(k_is_init, tblocks, kThreads, 0, s, t_key, t_cnt, t_lo, t_hi, tsize, flags);
  LGS_KLAUNCH(k_is_fold, (unsigned)((n + kFoldRows - 1) / kFoldRows), kThreads, 0, s, points, labels, instance_ids, n, scene_offsets, b, tail,
              t_key, t_cnt, t_lo, t_hi, tsize - 1, slot, flags, status);
  LGS_KLAUNCH(k_is_decide, tblocks, kThreads, 0, s, t_key, t_lo, t_hi, tsize, seg_cap, scene_bounds, tail, forced, color_prob, scale_prob,
              (uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), seeds, t_row, segs, flags);
  LGS_KLAUNCH(k_is_keys, rblocks, kThreads, 0, s, n, scene_offsets, b, seg_cap, t_row, flags, slot, keys, status);
  LGS_HIP(sort_rows(Layout::at<char>(workspace, w.tmp), tb, keys, skeys, srows, n, bits, s));
  LGS_KLAUNCH(k_is_apply, rblocks, kThreads, 0, s, points, colors, labels, instance_ids, n, srows, slot, segs, hue_as_written, points_out,
              colors_out, labels_out, instances_out, order);
  LGS_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
