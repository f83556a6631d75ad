// lgs_insttarget.hip -- the training targets of the instance-segmentation trainer on the device: the per-instance table of a batch
// (point count, box, centre) and the two offset losses with their gradient; gfx950.
//
// Replaces
//   downstream/insseg/datasets/dataset.py:280-304 (VoxelizationDataset.get_instance_info: per scene, in a DataLoader worker, one boolean
//   mask over all points per instance id), :336-341 (the ids of ignored labels become -1),
//   downstream/insseg/lib/pl_Trainer.py:280-284 (centers and ids concatenated over the batch and uploaded every step) and :286-298 (the
//   offset losses, about fifteen element-wise and reduction launches over [N, 3], forward and backward).
// An instance is the pair (batch index, id): the key (batch << 32) | id, both halves in [0, 2^31), so all ones names no key.
// lgs_instance_info, all on the caller's stream, no host synchronisation:
//   1. init     the table is emptied and the output rows are cleared (k_it_init).
//   2. fold     a workgroup combines its 2048 points in an LDS table of 512 entries (count, three 64-bit coordinate sums, min, max: LDS
//               integer atomics; a min / max is only sent when it improves on what the entry shows) and then adds every distinct key
//               ONCE to its entry of the global table (open addressing, table_claim): one set of global integer atomics per
//               (workgroup, distinct key), not one per point (k_it_fold).  A key that finds no LDS entry in 8 probes goes to the global
//               table directly.  The point remembers its global entry in slot[].
//   3. rows     an entry's output row is the rank of its key among the keys of the table, so the rows do not depend on which entry a
//               key happened to claim: every workgroup with an occupied entry walks the table, packs its occupied keys into LDS tile
//               by tile and counts the keys below its own (one loop step per INSTANCE, not per entry of the table).  k_it_rows then
//               moves the entry's statistics to its row and computes the centre.
//   4. points   slot[] goes from entry to row; centers[n, 3] is gathered from the table when asked for (k_it_points).
// Every sum is an integer, the centre is rounded from one fp64 quotient: the result does not depend on order, two calls give the same bits.
// lgs_offset_loss_forward / _backward: one streaming kernel each, fp32 per row, fp64 partial sums per workgroup in a fixed tree, the
// partials added in a fixed tree by one workgroup (k_ol_finish); the backward reads the upstream gradients and the valid count from the device.
#include <hip/hip_runtime.h>

#include "lgs_common.h"

namespace lgs {

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 8;
constexpr int kFoldPoints = kThreads * kPerThread;   // points per workgroup of the fold pass
constexpr int kLds = 512;                            // entries of its LDS table
constexpr int kLdsProbes = 8;
constexpr int kMaxMasked = 32;
constexpr int kMaxPartialRows = 1024;
constexpr unsigned long long kEmpty = ~0ull;
enum : int { kStOverflow = 1, kStIdRange = 2, kStBatch = 4 };

struct MaskList {
  int64_t v[kMaxMasked];
  int n;
};

__device__ inline uint32_t hash_key(unsigned long long h) {
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  return (uint32_t)h;
}

// stage 1
__global__ __launch_bounds__(kThreads) void k_it_init(unsigned long long *__restrict__ t_key, int32_t *__restrict__ t_cnt,
                                                      unsigned long long *__restrict__ t_sum, int32_t *__restrict__ t_min,
                                                      int32_t *__restrict__ t_max, uint32_t tsize, int inst_cap, int64_t *__restrict__ key,
                                                      int32_t *__restrict__ count, int32_t *__restrict__ bbox, float *__restrict__ center,
                                                      int32_t *__restrict__ status) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j == 0) *status = 0;
  if (j < tsize) {
    t_key[j] = kEmpty;
    t_cnt[j] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      t_sum[3 * (int64_t)j + a] = 0ull;
      t_min[3 * (int64_t)j + a] = INT32_MAX;
      t_max[3 * (int64_t)j + a] = INT32_MIN;
    }
  }
  if (j < (uint32_t)inst_cap) {
    key[j] = -1;
    count[j] = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) bbox[6 * (int64_t)j + a] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) center[3 * (int64_t)j + a] = 0.f;
  }
}

// add (c points, their coordinate sums s, their box lo .. hi) to entry e of a table in global memory
__device__ inline void global_merge(int32_t *__restrict__ t_cnt, unsigned long long *__restrict__ t_sum, int32_t *__restrict__ t_min,
                                    int32_t *__restrict__ t_max, int64_t e, int c, const unsigned long long *s, const int32_t *lo,
                                    const int32_t *hi) {
  atomicAdd(&t_cnt[e], c);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    atomicAdd(&t_sum[3 * e + a], s[a]);
    atomicMin(&t_min[3 * e + a], lo[a]);
    atomicMax(&t_max[3 * e + a], hi[a]);
  }
}

// stage 2
__global__ __launch_bounds__(kThreads) void k_it_fold(const int32_t *__restrict__ coords, const int64_t *__restrict__ ids,
                                                      const int64_t *__restrict__ labels, MaskList masked, int64_t n,
                                                      unsigned long long *__restrict__ t_key, int32_t *__restrict__ t_cnt,
                                                      unsigned long long *__restrict__ t_sum, int32_t *__restrict__ t_min,
                                                      int32_t *__restrict__ t_max, uint32_t tmask, int64_t *__restrict__ ids_out,
                                                      int32_t *__restrict__ slot, int32_t *__restrict__ status) {
  __shared__ unsigned long long l_key[kLds];
  __shared__ unsigned long long l_sum[kLds * 3];
  __shared__ int32_t l_cnt[kLds], l_min[kLds * 3], l_max[kLds * 3], l_entry[kLds];
  for (int j = threadIdx.x; j < kLds; j += kThreads) {
    l_key[j] = kEmpty;
    l_cnt[j] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      l_sum[3 * j + a] = 0ull;
      l_min[3 * j + a] = INT32_MAX;
      l_max[3 * j + a] = INT32_MIN;
    }
  }
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * kFoldPoints;
  int mine[kPerThread];                    // the LDS entry of my k-th point; -1: the point is done (no instance, or sent directly)
  int bad = 0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int64_t i = i0 + (int64_t)k * kThreads + threadIdx.x;
    mine[k] = -1;
    if (i >= n) continue;
    const int4 c = *reinterpret_cast<const int4 *>(coords + 4 * i);
    int64_t id = ids[i];
    if (id != -1 && labels) {
      const int64_t lab = labels[i];
      for (int q = 0; q < masked.n; ++q)
        if (lab == masked.v[q]) id = -1;
    }
    if (id != -1 && (id < 0 || id >= (1ll << 31))) { bad |= kStIdRange; id = -1; }
    if (id != -1 && c.x < 0) { bad |= kStBatch; id = -1; }
    ids_out[i] = id;
    if (id == -1) { slot[i] = -1; continue; }
    const unsigned long long key = ((unsigned long long)(uint32_t)c.x << 32) | (unsigned long long)id;
    const uint32_t hk = hash_key(key);
    const int32_t p[3] = {c.y, c.z, c.w};
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
        atomicAdd(&l_sum[3 * e + a], (unsigned long long)(long long)p[a]);
        // the entry only ever moves towards the extreme, so a value that does not improve on what it shows now never will
        if (p[a] < *(volatile int32_t *)&l_min[3 * e + a]) atomicMin(&l_min[3 * e + a], p[a]);
        if (p[a] > *(volatile int32_t *)&l_max[3 * e + a]) atomicMax(&l_max[3 * e + a], p[a]);
      }
    } else {
      const int64_t g = table_claim(t_key, hk & tmask, tmask, key, kEmpty, (uint64_t)tmask + 1);
      if (g >= 0) {
        const unsigned long long s[3] = {(unsigned long long)(long long)p[0], (unsigned long long)(long long)p[1], (unsigned long long)(long long)p[2]};
        global_merge(t_cnt, t_sum, t_min, t_max, g, 1, s, p, p);
      } else {
        bad |= kStOverflow;
      }
      slot[i] = (int32_t)g;
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < kLds; j += kThreads) {
    const unsigned long long key = l_key[j];
    if (key == kEmpty) continue;
    const int64_t g = table_claim(t_key, hash_key(key) & tmask, tmask, key, kEmpty, (uint64_t)tmask + 1);
    l_entry[j] = (int32_t)g;
    if (g >= 0) global_merge(t_cnt, t_sum, t_min, t_max, g, l_cnt[j], &l_sum[3 * j], &l_min[3 * j], &l_max[3 * j]);
    else bad |= kStOverflow;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int64_t i = i0 + (int64_t)k * kThreads + threadIdx.x;
    if (mine[k] >= 0) slot[i] = l_entry[mine[k]];
  }
  if (bad) atomicOr(status, bad);
}

// stage 3: an occupied entry's row is the number of keys in the table below its own (the empty key is above all); its statistics move there
constexpr int kRankTile = 2048;
__global__ __launch_bounds__(kThreads) void k_it_rows(const unsigned long long *__restrict__ t_key, const int32_t *__restrict__ t_cnt,
                                                      const unsigned long long *__restrict__ t_sum, const int32_t *__restrict__ t_min,
                                                      const int32_t *__restrict__ t_max, uint32_t tsize, int inst_cap,
                                                      int32_t *__restrict__ t_row, int64_t *__restrict__ key, int32_t *__restrict__ count,
                                                      int32_t *__restrict__ bbox, float *__restrict__ center, int32_t *__restrict__ status) {
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
    unsigned long long other[kRankTile / kThreads];      // every load issued before the first is used
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
  if (r >= (uint32_t)inst_cap) {
    atomicOr(status, (int)kStOverflow);
    return;
  }
  t_row[h] = (int32_t)r;
  key[r] = (int64_t)k;
  const int32_t c = t_cnt[h];
  count[r] = c;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    bbox[6 * (int64_t)r + a] = t_min[3 * (int64_t)h + a];
    bbox[6 * (int64_t)r + 3 + a] = t_max[3 * (int64_t)h + a];
    center[3 * (int64_t)r + a] = (float)((double)(long long)t_sum[3 * (int64_t)h + a] / (double)c);
  }
}

// stage 4
__global__ __launch_bounds__(kThreads) void k_it_points(int64_t n, const int32_t *__restrict__ t_row, const float *__restrict__ center,
                                                        int32_t *__restrict__ slot, float *__restrict__ centers) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t h = slot[i];
  const int32_t r = h >= 0 ? t_row[h] : -1;
  slot[i] = r;
  if (centers) {
#pragma unroll
    for (int a = 0; a < 3; ++a) centers[3 * i + a] = r >= 0 ? center[3 * (int64_t)r + a] : -1.f;
  }
}

// ---- the offset losses.  One row, in the reference's order, every operation rounded to fp32 (no contraction)
struct OffsetRow {
  float po[3], gt[3], diff[3];
  float gt_den, po_norm, po_den, dot;      // |gt| + 1e-8, |po|, |po| + 1e-8, gt_ . po_ (both sides over their denominators)
};
template <typename T>
__device__ inline OffsetRow offset_row(const T *__restrict__ po, const int32_t *__restrict__ coords, const float *__restrict__ center,
                                       int64_t r, int32_t s, float voxel) {
  OffsetRow o;
  const int4 c = *reinterpret_cast<const int4 *>(coords + 4 * r);
  const int32_t x[3] = {c.y, c.z, c.w};
  float gg = 0.f, pp = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    o.po[a] = ld_elem(po + 3 * r + a);
    o.gt[a] = __fmul_rn(__fsub_rn(center[3 * (int64_t)s + a], (float)x[a]), voxel);
    o.diff[a] = __fsub_rn(o.po[a], o.gt[a]);
    gg = __fadd_rn(gg, __fmul_rn(o.gt[a], o.gt[a]));
    pp = __fadd_rn(pp, __fmul_rn(o.po[a], o.po[a]));
  }
  o.gt_den = __fadd_rn(__fsqrt_rn(gg), 1e-8f);
  o.po_norm = __fsqrt_rn(pp);
  o.po_den = __fadd_rn(o.po_norm, 1e-8f);
  o.dot = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) o.dot = __fadd_rn(o.dot, __fmul_rn(__fdiv_rn(o.gt[a], o.gt_den), __fdiv_rn(o.po[a], o.po_den)));
  return o;
}

// -> partial[block][3] (fp64): the sums of the L1 distances, of the negative cosines and the number of rows with an instance.  The
// reduction of k_split_stats: per thread in row order, the wave in a butterfly, the four waves in order
template <typename T>
__global__ __launch_bounds__(kThreads) void k_ol_fwd(const T *__restrict__ po, const int32_t *__restrict__ coords,
                                                     const int32_t *__restrict__ slot, const float *__restrict__ center, int64_t n,
                                                     float voxel, double *__restrict__ partial) {
  __shared__ double l_acc[kThreads / 64][3];
  double acc[3] = {0.0, 0.0, 0.0};
  for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < n; r += (int64_t)gridDim.x * kThreads) {
    const int32_t s = slot[r];
    if (s < 0) continue;
    const OffsetRow o = offset_row(po, coords, center, r, s, voxel);
    const float dist = __fadd_rn(__fadd_rn(fabsf(o.diff[0]), fabsf(o.diff[1])), fabsf(o.diff[2]));
    acc[0] += (double)dist;
    acc[1] += (double)(-o.dot);
    acc[2] += 1.0;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[k] = wave_sum(acc[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) l_acc[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double a = l_acc[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) a += l_acc[w][threadIdx.x];
    partial[(int64_t)blockIdx.x * 3 + threadIdx.x] = a;
  }
}

// the partial rows of each column in a fixed tree: thread t takes the rows t, t + 256, ... in order, the wave folds in wave_sum's
// butterfly, the four waves are added in order; the losses are sum / (valid + 1e-6), rounded once
__global__ __launch_bounds__(kThreads) void k_ol_finish(const double *__restrict__ partial, int rows, float *__restrict__ norm_loss,
                                                        float *__restrict__ dir_loss, float *__restrict__ valid) {
  __shared__ double l_acc[kThreads / 64][3];
  double acc[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < rows; b += kThreads) {
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] += partial[(int64_t)b * 3 + k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[k] = wave_sum(acc[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) l_acc[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      sum[k] = l_acc[0][k];
#pragma unroll
      for (int w = 1; w < kThreads / 64; ++w) sum[k] += l_acc[w][k];
    }
    const double den = sum[2] + 1e-6;
    *norm_loss = (float)(sum[0] / den);
    *dir_loss = (float)(sum[1] / den);
    *valid = (float)sum[2];
  }
}

__device__ inline void st_elem(float *p, float v) { *p = v; }
__device__ inline void st_elem(bf16_t *p, float v) { *p = f32_to_bf16(v); }

// d po = g_norm / den * sign(po - gt) + g_dir / den * d(-(u . po) / D), den = valid + 1e-6, u = gt / (|gt| + 1e-8), D = |po| + 1e-8; zero
// without an instance.  With p^ = po / |po| and c = u . p^:
//   d(-(u . po) / D) / d po = -u / D + (u . po) p^ / D^2 = -((u - c p^) + c (1e-8 / D) p^) / D
// the part of u across po and the small part along it that the 1e-8 leaves, each computed on its own (added up as -u / D + ... the two
// terms cancel to 1e-8 / D of their size when po is parallel to gt).  At po == 0 the norm has torch's zero subgradient: -u / D.
template <typename T>
__global__ __launch_bounds__(kThreads) void k_ol_bwd(const T *__restrict__ po, const int32_t *__restrict__ coords,
                                                     const int32_t *__restrict__ slot, const float *__restrict__ center, int64_t n,
                                                     float voxel, const float *__restrict__ valid, const float *__restrict__ g_norm,
                                                     const float *__restrict__ g_dir, T *__restrict__ d_po) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= n) return;
  const int32_t s = slot[r];
  float g[3] = {0.f, 0.f, 0.f};
  if (s >= 0) {
    const float den = __fadd_rn(*valid, 1e-6f);
    const float a = __fdiv_rn(*g_norm, den), b = __fdiv_rn(*g_dir, den);
    const OffsetRow o = offset_row(po, coords, center, r, s, voxel);
    float u[3], ph[3], c = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      u[k] = __fdiv_rn(o.gt[k], o.gt_den);
      ph[k] = o.po_norm > 0.f ? __fdiv_rn(o.po[k], o.po_norm) : 0.f;
      c = __fmaf_rn(u[k], ph[k], c);
    }
    const float along = __fmul_rn(c, __fdiv_rn(1e-8f, o.po_den));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float sign = o.diff[k] > 0.f ? 1.f : (o.diff[k] < 0.f ? -1.f : 0.f);
      const float across = o.po_norm > 0.f ? __fmaf_rn(-c, ph[k], u[k]) : u[k];
      const float dir = -__fdiv_rn(__fmaf_rn(along, ph[k], across), o.po_den);
      g[k] = __fadd_rn(__fmul_rn(a, sign), __fmul_rn(b, dir));
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) st_elem(d_po + 3 * r + k, g[k]);
}

}  // namespace

}  // namespace lgs

using namespace lgs;

extern "C" int64_t lgs_instance_info_workspace_bytes(int64_t n, int inst_cap) {
  if (n < 0 || n >= (1ll << 31) || inst_cap < 1 || inst_cap > kInstTargetMaxCap) return -1;
  return inst_target_layout(inst_cap).total;
}

extern "C" int lgs_instance_info(const int32_t *coords, const int64_t *instance_ids, const int64_t *labels, int64_t n,
                                 const int64_t *masked_labels, int n_masked, int inst_cap, int64_t *ids_out, int32_t *slot, int64_t *key,
                                 int32_t *count, int32_t *bbox, float *center, float *centers, int32_t *status, void *workspace,
                                 void *stream) {
  LGS_REQUIRE(inst_cap >= 1 && inst_cap <= kInstTargetMaxCap, "lgs_instance_info: inst_cap must be in 1 .. 65536");
  LGS_REQUIRE(n >= 0 && n < (1ll << 31), "lgs_instance_info: n must be in 0 .. 2^31 - 1");
  LGS_REQUIRE(n_masked >= 0 && n_masked <= kMaxMasked, "lgs_instance_info: at most 32 masked labels");
  LGS_REQUIRE(n_masked == 0 || (masked_labels && labels), "lgs_instance_info: masked labels announced, no list or no labels given");
  LGS_REQUIRE(key && count && bbox && center && status && workspace, "lgs_instance_info: null output or workspace");
  LGS_REQUIRE(n == 0 || (coords && instance_ids && ids_out && slot), "lgs_instance_info: null point argument");
  hipStream_t s = (hipStream_t)stream;
  const uint32_t tsize = inst_target_table_size(inst_cap);
  const InstTargetWs w = inst_target_layout(inst_cap);
  unsigned long long *t_key = Layout::at<unsigned long long>(workspace, w.t_key), *t_sum = Layout::at<unsigned long long>(workspace, w.t_sum);
  int32_t *t_cnt = Layout::at<int32_t>(workspace, w.t_cnt), *t_min = Layout::at<int32_t>(workspace, w.t_min);
  int32_t *t_max = Layout::at<int32_t>(workspace, w.t_max), *t_row = Layout::at<int32_t>(workspace, w.t_row);
  MaskList masked;
  masked.n = n_masked;
  for (int q = 0; q < kMaxMasked; ++q) masked.v[q] = q < n_masked ? masked_labels[q] : 0;
  const unsigned tblocks = (tsize + kThreads - 1) / kThreads;     // tsize >= inst_cap
  LGS_KLAUNCH(k_it_init, tblocks, kThreads, 0, s, t_key, t_cnt, t_sum, t_min, t_max, tsize, inst_cap, key, count, bbox, center, status);
  if (n > 0) {
    LGS_KLAUNCH(k_it_fold, (unsigned)((n + kFoldPoints - 1) / kFoldPoints), kThreads, 0, s, coords, instance_ids, n_masked ? labels : nullptr,
                masked, n, t_key, t_cnt, t_sum, t_min, t_max, tsize - 1, ids_out, slot, status);
    LGS_KLAUNCH(k_it_rows, tblocks, kThreads, 0, s, t_key, t_cnt, t_sum, t_min, t_max, tsize, inst_cap, t_row, key, count, bbox, center, status);
    LGS_KLAUNCH(k_it_points, (unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, s, n, t_row, center, slot, centers);
  }
  LGS_HIP(hipGetLastError());
  return 0;
}

extern "C" int lgs_offset_loss_forward(const void *pt_offsets, const int32_t *coords, const int32_t *slot, const float *center, int64_t n,
                                       float voxel_size, int dtype, double *partial, int partial_rows, float *norm_loss, float *dir_loss,
                                       float *valid, void *stream) {
  LGS_REQUIRE(dtype == LGS_F32 || dtype == LGS_BF16, "lgs_offset_loss_forward: unknown dtype");
  LGS_REQUIRE(n >= 0 && n < (1ll << 31), "lgs_offset_loss_forward: n must be in 0 .. 2^31 - 1");
  LGS_REQUIRE(partial && partial_rows >= 1 && partial_rows <= kMaxPartialRows, "lgs_offset_loss_forward: partial_rows must be in 1 .. 1024");
  LGS_REQUIRE(norm_loss && dir_loss && valid, "lgs_offset_loss_forward: null output");
  LGS_REQUIRE(n == 0 || (pt_offsets && coords && slot && center), "lgs_offset_loss_forward: null input");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == LGS_BF16)
    LGS_KLAUNCH(k_ol_fwd<bf16_t>, (unsigned)partial_rows, kThreads, 0, s, reinterpret_cast<const bf16_t *>(pt_offsets), coords, slot, center, n,
                voxel_size, partial);
  else
    LGS_KLAUNCH(k_ol_fwd<float>, (unsigned)partial_rows, kThreads, 0, s, reinterpret_cast<const float *>(pt_offsets), coords, slot, center, n,
                voxel_size, partial);
  LGS_KLAUNCH(k_ol_finish, 1, kThreads, 0, s, partial, partial_rows, norm_loss, dir_loss, valid);
  LGS_HIP(hipGetLastError());
  return 0;
}

extern "C" int lgs_offset_loss_backward(const void *pt_offsets, const int32_t *coords, const int32_t *slot, const float *center, int64_t n,
                                        float voxel_size, int dtype, const float *valid, const float *g_norm, const float *g_dir,
                                        void *d_pt_offsets, void *stream) {
  LGS_REQUIRE(dtype == LGS_F32 || dtype == LGS_BF16, "lgs_offset_loss_backward: unknown dtype");
  LGS_REQUIRE(n >= 0 && n < (1ll << 31), "lgs_offset_loss_backward: n must be in 0 .. 2^31 - 1");
  LGS_REQUIRE(valid && g_norm && g_dir, "lgs_offset_loss_backward: null gradient or valid count");
  LGS_REQUIRE(n == 0 || (pt_offsets && coords && slot && center && d_pt_offsets), "lgs_offset_loss_backward: null input or output");
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((n + kThreads - 1) / kThreads);
  if (dtype == LGS_BF16)
    LGS_KLAUNCH(k_ol_bwd<bf16_t>, blocks, kThreads, 0, s, reinterpret_cast<const bf16_t *>(pt_offsets), coords, slot, center, n, voxel_size, valid,
                g_norm, g_dir, reinterpret_cast<bf16_t *>(d_pt_offsets));
  else
    LGS_KLAUNCH(k_ol_bwd<float>, blocks, kThreads, 0, s, reinterpret_cast<const float *>(pt_offsets), coords, slot, center, n, voxel_size, valid,
                g_norm, g_dir, reinterpret_cast<float *>(d_pt_offsets));
  LGS_HIP(hipGetLastError());
  return 0;
}
