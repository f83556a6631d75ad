// lgs_insteval.hip -- overlap tables of instance proposals against the ground-truth instances of one scene; gfx950.
//
// Replaces the device side of what the reference's instance evaluation does per scene on the host
//   downstream/insseg/lib/bfs/bfs.py:127-157 (one score_func over a boolean gather per proposal, three device -> host copies each),
//   downstream/insseg/datasets/evaluation/evaluate_semantic_instance.py:251-306 (assign_instances_for_scan: one full [N] pass per
//   (proposal, ground-truth instance of its class)), scannet_benchmark_utils/util_3d.py:154-165 (np.unique + one [N] pass per id)
// which is a segmented histogram of ground-truth ids over the cluster lists plus one reduction of a score column per proposal.
// Stages, all on the caller's stream, no host synchronisation:
//   1. ids      every point with a ground-truth instance id (id > 0 and id / 1000 among the valid classes) adds 1 to its id's entry of
//               an open-addressed table of T >= 2 g_cap entries in the workspace (64-bit atomicCAS on the key, 0 = empty: the id 0 names
//               no instance).  A workgroup first combines its 2048 points in an LDS table of 1024 entries and inserts each distinct id
//               once with its count (k_ie_ids); an id that finds no LDS entry in 8 probes goes to the global table directly.
//   2. slots    every occupied entry takes the next output slot: gt_id / gt_count, and the entry remembers its slot (k_ie_slots).
//   3. overlap  the hot pass.  Workgroup b owns the members [b kChunk, (b + 1) kChunk) of the flat member list, which is sorted by
//               proposal: it walks the pieces of proposals inside its chunk one after the other (several small proposals per workgroup,
//               several workgroups per big proposal).  Per member: one gather of gt_ids, one probe of the table, one LDS add into a
//               histogram of g_cap counters whose touched slots are listed, so that a piece clears and flushes only what it touched
//               (32-bit global adds into inter[q, :]: integer sums, order-free).  The member's score joins a per-thread maximum / fp64 sum;
//               the workgroup folds them in a fixed tree and writes ONE partial per piece, to slot b + q of the workspace (b and q
//               never both stand still from one piece to the next, so the slot is the piece's own).
//   4. conf     one thread per proposal folds its pieces' partials in chunk order and rounds once (k_ie_conf): no float atomics,
//               two calls give the same bits.  An empty proposal gets NaN.
#include <hip/hip_runtime.h>

#include "lgs_common.h"

namespace lgs {

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = kInstChunk;        // members per workgroup of the overlap pass (1024; the layout counts pieces by it)
constexpr int kIdPoints = 2048;           // points per workgroup of the id pass
constexpr int kIdLds = 1024;              // entries of its LDS table
constexpr int kIdProbes = 8;
constexpr int kMaxCap = 4096;
constexpr uint32_t kNanKey = 0xffffffffu;
enum : int { kStOverflow = 1, kStMember = 2, kStColumn = 4, kStClass = 8 };

__device__ inline uint32_t hash_id(int64_t g) {
  uint64_t h = (uint64_t)g;
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  return (uint32_t)h;
}
// ord_key with any NaN as the top key, whatever its sign: torch.max returns NaN once it meets one, so a NaN must win every maximum
__device__ inline uint32_t ord_of(float f) { return f != f ? kNanKey : ord_key(f); }
__device__ inline float of_ord(uint32_t o) { return o == kNanKey ? __uint_as_float(0x7fc00000u) : ord_key_inv(o); }
// g names an instance: g > 0 (a negative id floors to a negative class, and every valid class is >= 1) and g / 1000 is valid
__device__ inline bool is_instance(int64_t g, const int64_t *__restrict__ valid, int v) {
  if (g <= 0) return false;
  const int64_t cls = g / 1000;
  const int lo = lower_bound(valid, 0, v, cls);
  return lo < v && valid[lo] == cls;
}
// add `add` to g's entry of the global table (the key 0 = empty); false = no entry left in T probes
__device__ inline bool table_add(unsigned long long *__restrict__ t_key, int32_t *__restrict__ t_cnt, uint32_t tmask, int64_t g, int add) {
  const int64_t h = table_claim(t_key, hash_id(g) & tmask, tmask, (unsigned long long)g, 0ull, (uint64_t)tmask + 1);
  if (h >= 0) atomicAdd(&t_cnt[h], add);
  return h >= 0;
}

// stage 1
__global__ __launch_bounds__(kThreads) void k_ie_ids(const int64_t *__restrict__ gt_ids, int64_t n, const int64_t *__restrict__ valid, int v,
                                                     unsigned long long *__restrict__ t_key, int32_t *__restrict__ t_cnt, uint32_t tmask,
                                                     int32_t *__restrict__ status) {
  __shared__ unsigned long long l_key[kIdLds];
  __shared__ int32_t l_cnt[kIdLds];
  for (int j = threadIdx.x; j < kIdLds; j += kThreads) { l_key[j] = 0ull; l_cnt[j] = 0; }
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * kIdPoints, i1 = i0 + kIdPoints < n ? i0 + kIdPoints : n;
  bool lost = false;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += kThreads) {
    const int64_t g = gt_ids[i];
    if (!is_instance(g, valid, v)) continue;
    // table_claim's probe sequence on the LDS table, spelled out: through the helper the kernel measured slower (profiles/device_idioms.md)
    uint32_t h = hash_id(g) & (kIdLds - 1);
    bool placed = false;
#pragma unroll 1
    for (int probe = 0; probe < kIdProbes && !placed; ++probe) {
      const unsigned long long prev = atomicCAS(&l_key[h], 0ull, (unsigned long long)g);
      if (prev == 0ull || prev == (unsigned long long)g) {
        atomicAdd(&l_cnt[h], 1);
        placed = true;
      }
      h = (h + 1) & (kIdLds - 1);
    }
    if (!placed) lost |= !table_add(t_key, t_cnt, tmask, g, 1);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < kIdLds; j += kThreads)
    if (l_key[j] != 0ull) lost |= !table_add(t_key, t_cnt, tmask, (int64_t)l_key[j], l_cnt[j]);
  if (lost) atomicOr(status, (int)kStOverflow);
}

// stage 2: an occupied entry takes the next slot (t_cnt becomes the slot, -1 beyond g_cap); the valid class ids are checked on the way
__global__ __launch_bounds__(kThreads) void k_ie_slots(const unsigned long long *__restrict__ t_key, int32_t *__restrict__ t_cnt, uint32_t tsize,
                                                       int g_cap, int32_t *__restrict__ n_slots, int64_t *__restrict__ gt_id,
                                                       int32_t *__restrict__ gt_count, const int64_t *__restrict__ valid, int v,
                                                       int32_t *__restrict__ status) {
  const uint32_t h = blockIdx.x * kThreads + threadIdx.x;
  if (h < (uint32_t)v && valid[h] < 1) atomicOr(status, (int)kStClass);
  if (h >= tsize || t_key[h] == 0ull) return;
  const int slot = atomicAdd(n_slots, 1);
  if (slot < g_cap) {
    gt_id[slot] = (int64_t)t_key[h];
    gt_count[slot] = t_cnt[h];
    t_cnt[h] = slot;
  } else {
    t_cnt[h] = -1;
    atomicOr(status, (int)kStOverflow);
  }
}

// stage 3.  MODE: 0 none, 1 max, 2 mean
template <typename T, int MODE>
__global__ __launch_bounds__(kThreads) void k_ie_overlap(const int32_t *__restrict__ member, int64_t m, const int32_t *__restrict__ offsets,
                                                         const int32_t *__restrict__ score_col, int p, const int64_t *__restrict__ gt_ids,
                                                         int64_t n, const T *__restrict__ scores, int c,
                                                         const unsigned long long *__restrict__ t_key, const int32_t *__restrict__ t_slot,
                                                         uint32_t tmask, int g_cap, int32_t *__restrict__ inter,
                                                         int32_t *__restrict__ prop_void, uint32_t *__restrict__ part_max,
                                                         double *__restrict__ part_sum, int32_t *__restrict__ status) {
  __shared__ int32_t l_hist[kMaxCap];
  __shared__ int32_t l_touched[kChunk];     // a piece has at most kChunk members, so at most that many slots
  __shared__ int32_t l_ntouched, l_void;
  __shared__ uint32_t l_wmax[kThreads / 64];
  __shared__ double l_wsum[kThreads / 64];
  for (int j = threadIdx.x; j < g_cap; j += kThreads) l_hist[j] = 0;
  if (threadIdx.x == 0) { l_ntouched = 0; l_void = 0; }
  const int64_t j0 = (int64_t)blockIdx.x * kChunk, j1 = j0 + kChunk < m ? j0 + kChunk : m;
  // the proposal of member j0: the first q with offsets[q + 1] > j0 (proposals in front of it that are empty are skipped)
  // (upper_bound over offsets + 1 and the wave folds below, spelled out: through the helpers the kernel measured slower)
  int q;
  {
    int lo = 0, hi = p;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)offsets[mid + 1] <= j0) lo = mid + 1; else hi = mid;
    }
    q = lo;
  }
  __syncthreads();
  int bad = 0;
  for (int64_t j = j0; j < j1 && q < p; ++q) {
    const int64_t qend = offsets[q + 1];
    if (qend <= j) continue;                 // an empty proposal
    const int64_t end = qend < j1 ? qend : j1;
    int col = 0;
    if (MODE != 0) {
      col = score_col[q];
      if (col < 0 || col >= c) { col = -1; bad |= kStColumn; }
    }
    int nvoid = 0;
    uint32_t mx = 0;                         // below every key of a float
    double sum = 0.0;
    for (int64_t k = j + threadIdx.x; k < end; k += kThreads) {
      const int64_t idx = member[k];
      if (idx < 0 || idx >= n) { bad |= kStMember; continue; }
      const int64_t g = gt_ids ? gt_ids[idx] : 0;      // no ground truth: every member is void
      int slot = -2;                         // -2 void, -1 an id beyond g_cap (overflow: flagged by stage 2)
      if (g != 0) {
        uint32_t h = hash_id(g) & tmask;
        for (uint32_t probe = 0; probe <= tmask; ++probe) {
          const unsigned long long key = t_key[h];
          if (key == (unsigned long long)g) { slot = t_slot[h]; break; }
          if (key == 0ull) break;
          h = (h + 1) & tmask;
        }
      }
      if (slot >= 0) {
        if (atomicAdd(&l_hist[slot], 1) == 0) l_touched[atomicAdd(&l_ntouched, 1)] = slot;
      } else if (slot == -2) {
        ++nvoid;
      }
      if (MODE != 0 && col >= 0) {
        const float x = ld_elem(scores + idx * c + col);
        if (MODE == 1) { const uint32_t o = ord_of(x); mx = o > mx ? o : mx; }
        else sum += (double)x;
      }
    }
    // fold: the wave in a butterfly, the four waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      nvoid += __shfl_xor(nvoid, o, 64);
      if (MODE == 1) { const uint32_t ov = __shfl_xor(mx, o, 64); mx = ov > mx ? ov : mx; }
      if (MODE == 2) sum += __shfl_xor(sum, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      if (nvoid) atomicAdd(&l_void, nvoid);
      if (MODE == 1) l_wmax[threadIdx.x >> 6] = mx;
      if (MODE == 2) l_wsum[threadIdx.x >> 6] = sum;
    }
    __syncthreads();
    const int nt = l_ntouched;
    for (int t = threadIdx.x; t < nt; t += kThreads) {
      const int slot = l_touched[t];
      atomicAdd(&inter[(int64_t)q * g_cap + slot], l_hist[slot]);
      l_hist[slot] = 0;
    }
    if (threadIdx.x == 0) {
      if (l_void) atomicAdd(&prop_void[q], l_void);
      const int64_t piece = (int64_t)blockIdx.x + q;
      if (MODE == 1) {
        uint32_t a = l_wmax[0];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) a = l_wmax[w] > a ? l_wmax[w] : a;
        part_max[piece] = a;
      }
      if (MODE == 2) {
        double a = l_wsum[0];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) a += l_wsum[w];
        part_sum[piece] = a;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) { l_ntouched = 0; l_void = 0; }
    __syncthreads();
    j = end;
    if (end < qend) break;                   // the proposal goes on in the next workgroup's chunk
  }
  if (bad) atomicOr(status, bad);
}

// stage 4: proposal q's pieces are the chunks first .. last of its member range, at slots chunk + q
template <int MODE>
__global__ __launch_bounds__(kThreads) void k_ie_conf(const int32_t *__restrict__ offsets, int64_t m, const int32_t *__restrict__ score_col, int p, int c,
                                                      const uint32_t *__restrict__ part_max, const double *__restrict__ part_sum,
                                                      float *__restrict__ conf) {
  const int q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= p) return;
  const int64_t lo = offsets[q], hi = offsets[q + 1];
  const int col = score_col[q];
  if (hi <= lo || lo < 0 || hi > m || col < 0 || col >= c) {
    conf[q] = __uint_as_float(0x7fc00000u);
    return;
  }
  const int64_t b0 = lo / kChunk, b1 = (hi - 1) / kChunk;
  if (MODE == 1) {
    uint32_t a = 0;
    for (int64_t b = b0; b <= b1; ++b) a = part_max[b + q] > a ? part_max[b + q] : a;
    conf[q] = of_ord(a);
  } else {
    double a = 0.0;
    for (int64_t b = b0; b <= b1; ++b) a += part_sum[b + q];
    conf[q] = (float)(a / (double)(hi - lo));
  }
}

}  // namespace

}  // namespace lgs

using namespace lgs;

extern "C" int64_t lgs_inst_overlap_workspace_bytes(int64_t n, int64_t m, int p, int g_cap) {
  if (n < 0 || m < 0 || p < 0 || g_cap < 1 || g_cap > kMaxCap) return -1;
  return inst_overlap_layout(m, p, g_cap).total;
}

extern "C" int lgs_inst_overlap(const int32_t *member, const int32_t *offsets, const int32_t *score_col, int p, int64_t m,
                                const int64_t *gt_ids, int64_t n, const int64_t *valid_class_ids, int v, const void *scores, int c, int dtype,
                                int score_mode, int g_cap, int64_t *gt_id, int32_t *gt_count, int32_t *inter, int32_t *prop_void, float *conf,
                                int32_t *status, void *workspace, void *stream) {
  LGS_REQUIRE(g_cap >= 1 && g_cap <= kMaxCap, "lgs_inst_overlap: g_cap must be in 1 .. 4096");
  LGS_REQUIRE(n >= 0 && m >= 0 && p >= 0 && v >= 0, "lgs_inst_overlap: negative size");
  LGS_REQUIRE(n < (1ll << 31) && m < (1ll << 31), "lgs_inst_overlap: more points or members than a 32-bit index holds");
  LGS_REQUIRE(score_mode >= 0 && score_mode <= 2, "lgs_inst_overlap: score_mode must be 0 (none), 1 (max) or 2 (mean)");
  LGS_REQUIRE(gt_id && gt_count && status && workspace, "lgs_inst_overlap: null output or workspace");
  LGS_REQUIRE(p == 0 || (offsets && inter && prop_void), "lgs_inst_overlap: null proposal argument");
  LGS_REQUIRE(m == 0 || (member && p > 0), "lgs_inst_overlap: members without proposals");
  LGS_REQUIRE(!gt_ids || valid_class_ids || v == 0, "lgs_inst_overlap: v valid class ids announced, none given");
  if (score_mode != 0) {
    LGS_REQUIRE(dtype == LGS_F32 || dtype == LGS_BF16, "lgs_inst_overlap: unknown dtype");
    LGS_REQUIRE(p == 0 || (score_col && conf), "lgs_inst_overlap: score_mode without score_col / conf");
    LGS_REQUIRE(m == 0 || (scores && c >= 1), "lgs_inst_overlap: score_mode without scores");
  }
  hipStream_t s = (hipStream_t)stream;
  const uint32_t tsize = inst_table_size(g_cap);
  const InstOverlapWs w = inst_overlap_layout(m, p, g_cap);
  unsigned long long *t_key = Layout::at<unsigned long long>(workspace, w.t_key);
  int32_t *t_cnt = Layout::at<int32_t>(workspace, w.t_cnt), *n_slots = Layout::at<int32_t>(workspace, w.n_slots);
  uint32_t *part_max = Layout::at<uint32_t>(workspace, w.part_max);
  double *part_sum = Layout::at<double>(workspace, w.part_sum);
  LGS_HIP(hipMemsetAsync(workspace, 0, (size_t)w.zeroed, s));
  LGS_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
  LGS_HIP(hipMemsetAsync(gt_id, 0, sizeof(int64_t) * g_cap, s));
  LGS_HIP(hipMemsetAsync(gt_count, 0, sizeof(int32_t) * g_cap, s));
  if (p > 0) {
    LGS_HIP(hipMemsetAsync(inter, 0, sizeof(int32_t) * (size_t)p * g_cap, s));
    LGS_HIP(hipMemsetAsync(prop_void, 0, sizeof(int32_t) * (size_t)p, s));
  }
  if (n > 0 && gt_ids) LGS_KLAUNCH(k_ie_ids, (unsigned)((n + kIdPoints - 1) / kIdPoints), kThreads, 0, s, gt_ids, n, valid_class_ids, v, t_key, t_cnt, tsize - 1, status);
  const uint32_t slot_threads = tsize > (uint32_t)v ? tsize : (uint32_t)v;
  LGS_KLAUNCH(k_ie_slots, (slot_threads + kThreads - 1) / kThreads, kThreads, 0, s, t_key, t_cnt, tsize, g_cap, n_slots, gt_id, gt_count,
              valid_class_ids, v, status);
  if (m > 0) {
    const unsigned blocks = (unsigned)((m + kChunk - 1) / kChunk);
#define LGS_IE_OVERLAP(T, MODE)                                                                                                          \
  LGS_KLAUNCH((k_ie_overlap<T, MODE>), blocks, kThreads, 0, s, member, m, offsets, score_col, p, gt_ids, n, reinterpret_cast<const T *>(scores), \
              c, t_key, t_cnt, tsize - 1, g_cap, inter, prop_void, part_max, part_sum, status)
    if (score_mode == 0) LGS_IE_OVERLAP(float, 0);
    else if (dtype == LGS_BF16 && score_mode == 1) LGS_IE_OVERLAP(bf16_t, 1);
    else if (dtype == LGS_BF16) LGS_IE_OVERLAP(bf16_t, 2);
    else if (score_mode == 1) LGS_IE_OVERLAP(float, 1);
    else LGS_IE_OVERLAP(float, 2);
#undef LGS_IE_OVERLAP
  }
  if (score_mode != 0 && p > 0) {
    if (score_mode == 1) LGS_KLAUNCH(k_ie_conf<1>, (unsigned)((p + kThreads - 1) / kThreads), kThreads, 0, s, offsets, m, score_col, p, c, part_max, part_sum, conf);
    else LGS_KLAUNCH(k_ie_conf<2>, (unsigned)((p + kThreads - 1) / kThreads), kThreads, 0, s, offsets, m, score_col, p, c, part_max, part_sum, conf);
  }
  LGS_HIP(hipGetLastError());
  return 0;
}
