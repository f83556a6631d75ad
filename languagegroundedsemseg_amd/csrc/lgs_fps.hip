// lgs_fps.hip -- furthest point sampling over CSR segments: the limited-annotation subsets on the device, gfx950.
//
// Replaces furthest_point_sample (lib/ext/pointnet2/_ext_src/src/sampling_gpu.cu:75-178) as lib/datasets/preprocessing/
// scannet_long.py:98-109 calls it: per annotated instance, max(5, round(ratio * n)) samples of the instance's n points.  One segment
// is one chain of m dependent arg-max rounds (the contract is in include/lgs_engine.h); a call runs many segments side by side.
//
// Every tier runs the same round.  A thread owns the points k = tid, tid + T, ... of its segment (T = the threads that share the
// segment).  Per round it folds the winner of the round before into its t[k] and keeps its best point as a 64-bit key
// (bits of t) << 32 | ~k with the point's coordinates and row: t >= 0 orders as an unsigned integer and the complement sends equal
// t to the smallest k.  An ineligible point has key 0, below every eligible one.  A 6-step xor butterfly gives the wave's maximum;
// the one lane that holds it owns the winner.  What differs between the tiers is where the state lives and how waves meet:
//   k_fps_wave      n <= 256: one wave per segment, four segments per workgroup.  x, y, z, t and the row of four points per lane in
//                   registers; the winner's coordinates come by lane read.  No LDS, no barrier: a round is bounded by the 4 distance
//                   updates, the butterfly (12 cross-lane moves of 32 bits) and 3 lane reads.
//   k_fps_group     n <= 2048 with 4 waves, n <= 8192 with 16: one workgroup per segment, eight points per thread in registers.  The
//                   owning lane of each wave writes (key, x, y, z) to the wave's slot of a parity-double-buffered LDS table; one
//                   barrier; every wave folds the slots itself (log2(waves) butterfly steps) and reads the winner's coordinates from
//                   its slot, so there is no LDS copy of the cloud and no second barrier.  A round is bounded by the barrier and two
//                   LDS round trips on top of the wave tier's work.
//   k_fps_stream    larger: one workgroup of 16 waves per segment.  (x, y, z, t) per position as one 16-byte record in the workspace,
//                   staged once, read every round, t written back only where it fell; the meeting of the waves is k_fps_group's.  A
//                   round is bounded by one workgroup's read of 16 n bytes from L2 (100 k points = 1.6 MB, resident in one XCD's L2).
// The key is a total order over the segment's points, so the maximum does not depend on how points are dealt to lanes, waves or
// tiers: the result is a function of the segment alone, whatever the tier, grid or workgroup size, and two calls give the same bits.
// rank_out takes unsigned integer minima, so rows that several segments share through `through` end the same way in any order.
// Launches of one call, in stream order: k_fps_fill (rank_out = -1), k_fps_table (the clamped segment table, the counts, the
// output offsets), then the four round kernels, each over all segments: a workgroup (a wave in k_fps_wave) whose segment belongs
// to another tier leaves at once.  Nothing is read back.
//
// Deviation from the reference: it resolves exact ties in a round's maximum by its block-strided reduction tree,
// so its tie order depends on its block size; here ties go to the smallest index.  The two are equal on every input without an exact
// tie and after exhaustion.
#include <algorithm>
#include <cmath>

#include "lgs_common.h"

namespace lgs {

namespace {

#pragma clang fp contract(off)

constexpr int kFpsWaveMax = LGS_FPS_WAVE_MAX;          // largest segment of k_fps_wave
constexpr int kFpsGroup4Max = LGS_FPS_GROUP4_MAX;      // ... of k_fps_group with 4 waves
constexpr int kFpsGroup16Max = LGS_FPS_GROUP16_MAX;    // ... with 16 waves
constexpr int kFpsWavePer = kFpsWaveMax / 64;          // points per lane
constexpr int kFpsGroupPer = 8;                        // points per thread
static_assert(kFpsGroup4Max == 4 * 64 * kFpsGroupPer && kFpsGroup16Max == 16 * 64 * kFpsGroupPer, "tier bounds are whole register files");
constexpr int kFpsStreamWaves = 16;
constexpr int kFpsStreamBatch = 8;                     // records a thread of k_fps_stream loads before it uses the first
constexpr int kFpsTableBlock = 1024;
constexpr float kFpsFar = 1e10f;

struct FpsSeg {            // one per segment, in the workspace
  int64_t lo;              // first position
  int64_t out;             // first entry of idx_out
  int32_t n, m;
};
static_assert(sizeof(FpsSeg) == kFpsSegBytes, "fps_layout sizes the segment records");

struct FpsSlot {           // what a wave brings to the meeting
  unsigned long long key;
  float x, y, z;
  int32_t pad;
};

__device__ inline float fps_dist(float x, float y, float z, float xo, float yo, float zo) {
  const float dx = x - xo, dy = y - yo, dz = z - zo;
  return (dx * dx + dy * dy) + dz * dz;
}
__device__ inline bool fps_eligible(float x, float y, float z, int skip_origin) { return !skip_origin || (x * x + y * y) + z * z > 1e-3f; }
__device__ inline unsigned long long fps_key(float t, uint32_t k) { return ((unsigned long long)__float_as_uint(t) << 32) | (uint32_t)~k; }
__device__ inline uint32_t fps_key_point(unsigned long long key) { return ~(uint32_t)key; }
// the row of position u (a row outside the table is clamped into it: nothing is read out of bounds)
__device__ inline int64_t fps_row(const int64_t *__restrict__ through, int64_t n, int64_t u) {
  return through ? std::min(std::max(through[u], (int64_t)0), n - 1) : u;
}

__global__ void k_fps_fill(int32_t *__restrict__ rank_out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) rank_out[i] = -1;
}

// the segment table: offsets clamped into a non-decreasing table on [0, n] (a running maximum), counts, output offsets.  One workgroup.
__global__ void __launch_bounds__(kFpsTableBlock) k_fps_table(const int64_t *__restrict__ seg_offsets, int64_t n, int64_t s,
                                                              const int32_t *__restrict__ counts, int fixed_count, double ratio,
                                                              int min_points, const int64_t *__restrict__ out_offsets,
                                                              FpsSeg *__restrict__ segs) {
  __shared__ int64_t sh[kFpsTableBlock];
  const int64_t per = (s + 1 + kFpsTableBlock - 1) / kFpsTableBlock, first = per * threadIdx.x, last = std::min(first + per, s + 1);
  int64_t mine = 0;
  for (int64_t q = first; q < last; ++q) mine = std::max(mine, seg_offsets[q]);
  sh[threadIdx.x] = mine;
  __syncthreads();
  for (int o = 1; o < kFpsTableBlock; o <<= 1) {      // inclusive running maximum over the threads
    const int64_t u = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
    __syncthreads();
    sh[threadIdx.x] = std::max(sh[threadIdx.x], u);
    __syncthreads();
  }
  int64_t run = threadIdx.x ? sh[threadIdx.x - 1] : 0;
  for (int64_t q = first; q < last; ++q) {
    run = std::max(run, seg_offsets[q]);
    const int64_t lo = std::min(run, n);
    if (q == s) break;
    const int64_t hi = std::min(std::max(run, seg_offsets[q + 1]), n);
    FpsSeg g;
    g.lo = lo;
    g.n = (int32_t)(hi - lo);
    int64_t m;
    if (counts) m = std::max(counts[q], 0);
    else if (fixed_count >= 0) m = fixed_count;
    else m = std::max((int64_t)min_points, (int64_t)rint(__dmul_rn(ratio, (double)g.n)));
    g.m = g.n ? (int32_t)std::min<int64_t>(m, LGS_FPS_MAX_SAMPLES) : 0;
    g.out = out_offsets ? out_offsets[q] : q * (int64_t)std::max(fixed_count, 0);
    segs[q] = g;
  }
}

// what the winner's owner leaves behind for round j
__device__ inline void fps_emit(int32_t *__restrict__ idx_out, int32_t *__restrict__ rank_out, int64_t out, int32_t j, uint32_t k,
                                int64_t row) {
  if (idx_out) idx_out[out + j] = (int32_t)k;
  if (rank_out) atomicMin(reinterpret_cast<unsigned int *>(rank_out) + row, (unsigned int)j);
}

// The meeting of WAVES waves: `best` is this lane's key (0 = none) with its coordinates; -> the segment's maximum, its coordinates in
// (xo, yo, zo) when it is not 0.  One barrier; `par` names the half of the slot table this round writes.
template <int WAVES>
__device__ inline unsigned long long fps_meet(unsigned long long best, float bx, float by, float bz, FpsSlot (*slots)[WAVES], int &par,
                                              float &xo, float &yo, float &zo) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long wbest = wave_max(best);
  if (wbest ? best == wbest : lane == 0) {         // keys differ between points: one lane
    FpsSlot &d = slots[par][wave];
    d.key = wbest; d.x = bx; d.y = by; d.z = bz;
  }
  __syncthreads();
  const unsigned long long all = wave_fold<WAVES>(slots[par][lane & (WAVES - 1)].key,
                                                  [](unsigned long long a, unsigned long long b) { return b > a ? b : a; });
  if (all) {
    const FpsSlot &w = slots[par][(fps_key_point(all) & (WAVES * 64 - 1)) >> 6];      // point k lives in thread k mod T
    xo = w.x; yo = w.y; zo = w.z;
  }
  par ^= 1;
  return all;
}

// one wave per segment: segment 4 * blockIdx.x + wave
__global__ void __launch_bounds__(256) k_fps_wave(const float *__restrict__ points, int64_t n, const int64_t *__restrict__ through,
                                                  const FpsSeg *__restrict__ segs, int64_t s, int skip_origin,
                                                  int32_t *__restrict__ idx_out, int32_t *__restrict__ rank_out) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= s) return;
  const FpsSeg g = segs[q];
  if (g.m <= 0 || g.n > kFpsWaveMax) return;       // wave-uniform
  float x[kFpsWavePer], y[kFpsWavePer], z[kFpsWavePer], t[kFpsWavePer];
  int32_t row[kFpsWavePer];
  uint32_t eligible = 0;
#pragma unroll
  for (int i = 0; i < kFpsWavePer; ++i) {
    const int k = i * 64 + lane;
    const int64_t r = fps_row(through, n, g.lo + std::min(k, g.n - 1));
    x[i] = points[3 * r]; y[i] = points[3 * r + 1]; z[i] = points[3 * r + 2];
    row[i] = (int32_t)r;
    t[i] = kFpsFar;
    if (k < g.n && fps_eligible(x[i], y[i], z[i], skip_origin)) eligible |= 1u << i;
  }
  const float x0 = __shfl(x[0], 0), y0 = __shfl(y[0], 0), z0 = __shfl(z[0], 0);
  float xo = x0, yo = y0, zo = z0;
  if (lane == 0) fps_emit(idx_out, rank_out, g.out, 0, 0u, row[0]);
  for (int32_t j = 1; j < g.m; ++j) {
    unsigned long long best = 0;
    float bx = x0, by = y0, bz = z0;
    int32_t brow = row[0];
#pragma unroll
    for (int i = 0; i < kFpsWavePer; ++i) {
      if ((eligible >> i) & 1u) {
        t[i] = fminf(fps_dist(x[i], y[i], z[i], xo, yo, zo), t[i]);
        const unsigned long long key = fps_key(t[i], (uint32_t)(i * 64 + lane));
        if (key > best) { best = key; bx = x[i]; by = y[i]; bz = z[i]; brow = row[i]; }
      }
    }
    const unsigned long long all = wave_max(best);
    const int src = all ? (int)(fps_key_point(all) & 63u) : 0;      // no eligible point: point 0, which lane 0 holds
    xo = __shfl(bx, src); yo = __shfl(by, src); zo = __shfl(bz, src);
    if (lane == src) fps_emit(idx_out, rank_out, g.out, j, all ? fps_key_point(all) : 0u, brow);
  }
}

// one workgroup of WAVES waves per segment, the state in registers
template <int WAVES>
__global__ void __launch_bounds__(WAVES * 64) k_fps_group(const float *__restrict__ points, int64_t n, const int64_t *__restrict__ through,
                                                          const FpsSeg *__restrict__ segs, int above, int upto, int skip_origin,
                                                          int32_t *__restrict__ idx_out, int32_t *__restrict__ rank_out) {
  constexpr int T = WAVES * 64, P = kFpsGroupPer;
  __shared__ FpsSlot slots[2][WAVES];
  const FpsSeg g = segs[blockIdx.x];
  if (g.m <= 0 || g.n <= above || g.n > upto) return;      // block-uniform
  const int tid = threadIdx.x;
  float x[P], y[P], z[P], t[P];
  int32_t row[P];
  uint32_t eligible = 0;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int k = i * T + tid;
    const int64_t r = fps_row(through, n, g.lo + std::min(k, g.n - 1));
    x[i] = points[3 * r]; y[i] = points[3 * r + 1]; z[i] = points[3 * r + 2];
    row[i] = (int32_t)r;
    t[i] = kFpsFar;
    if (k < g.n && fps_eligible(x[i], y[i], z[i], skip_origin)) eligible |= 1u << i;
  }
  const int64_t r0 = fps_row(through, n, g.lo);
  const float x0 = points[3 * r0], y0 = points[3 * r0 + 1], z0 = points[3 * r0 + 2];
  float xo = x0, yo = y0, zo = z0;
  int par = 0;
  if (tid == 0) fps_emit(idx_out, rank_out, g.out, 0, 0u, r0);
  for (int32_t j = 1; j < g.m; ++j) {
    unsigned long long best = 0;
    float bx = x0, by = y0, bz = z0;
    int32_t brow = (int32_t)r0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
      if ((eligible >> i) & 1u) {
        t[i] = fminf(fps_dist(x[i], y[i], z[i], xo, yo, zo), t[i]);
        const unsigned long long key = fps_key(t[i], (uint32_t)(i * T + tid));
        if (key > best) { best = key; bx = x[i]; by = y[i]; bz = z[i]; brow = row[i]; }
      }
    }
    const unsigned long long all = fps_meet<WAVES>(best, bx, by, bz, slots, par, xo, yo, zo);
    if (!all) { xo = x0; yo = y0; zo = z0; }               // no eligible point: point 0
    if (all ? best == all : tid == 0) fps_emit(idx_out, rank_out, g.out, j, all ? fps_key_point(all) : 0u, brow);
  }
}

// one workgroup per segment, the state in the workspace: state[u] = (x, y, z, t) of position u, t < 0 on an ineligible point
__global__ void __launch_bounds__(kFpsStreamWaves * 64) k_fps_stream(const float *__restrict__ points, int64_t n,
                                                                     const int64_t *__restrict__ through, const FpsSeg *__restrict__ segs,
                                                                     int above, int skip_origin, float4 *__restrict__ state,
                                                                     int32_t *__restrict__ idx_out, int32_t *__restrict__ rank_out) {
  constexpr int T = kFpsStreamWaves * 64;
  __shared__ FpsSlot slots[2][kFpsStreamWaves];
  const FpsSeg g = segs[blockIdx.x];
  if (g.m <= 0 || g.n <= above) return;                    // block-uniform
  const int tid = threadIdx.x;
  float4 *st = state + g.lo;
  for (int k = tid; k < g.n; k += T) {                     // a thread reads back only what it wrote itself: no barrier
    const int64_t r = fps_row(through, n, g.lo + k);
    const float x = points[3 * r], y = points[3 * r + 1], z = points[3 * r + 2];
    st[k] = make_float4(x, y, z, fps_eligible(x, y, z, skip_origin) ? kFpsFar : -1.f);
  }
  const int64_t r0 = fps_row(through, n, g.lo);
  const float x0 = points[3 * r0], y0 = points[3 * r0 + 1], z0 = points[3 * r0 + 2];
  float xo = x0, yo = y0, zo = z0;
  int par = 0;
  if (tid == 0) fps_emit(idx_out, rank_out, g.out, 0, 0u, r0);
  for (int32_t j = 1; j < g.m; ++j) {
    unsigned long long best = 0;
    float bx = x0, by = y0, bz = z0;
    for (uint32_t base = tid; base < (uint32_t)g.n; base += kFpsStreamBatch * T) {
      // The loads of a batch are in flight together: a round is latency first.  They are unconditional (a record past the end
      // reads the segment's last one and is dropped below): behind a branch each load is waited for before the next is issued.
      float4 v[kFpsStreamBatch];
#pragma unroll
      for (int u = 0; u < kFpsStreamBatch; ++u) v[u] = st[std::min(base + u * T, (uint32_t)g.n - 1u)];
#pragma unroll
      for (int u = 0; u < kFpsStreamBatch; ++u) {
        const uint32_t k = base + u * T;
        if (k < (uint32_t)g.n && v[u].w >= 0.f) {
          const float tn = fminf(fps_dist(v[u].x, v[u].y, v[u].z, xo, yo, zo), v[u].w);
          if (tn < v[u].w) st[k].w = tn;
          const unsigned long long key = fps_key(tn, k);
          if (key > best) { best = key; bx = v[u].x; by = v[u].y; bz = v[u].z; }
        }
      }
    }
    const unsigned long long all = fps_meet<kFpsStreamWaves>(best, bx, by, bz, slots, par, xo, yo, zo);
    if (!all) { xo = x0; yo = y0; zo = z0; }
    if (all ? best == all : tid == 0) {
      const uint32_t k = all ? fps_key_point(all) : 0u;
      fps_emit(idx_out, rank_out, g.out, j, k, fps_row(through, n, g.lo + k));
    }
  }
}

inline bool fps_shape_ok(int64_t n, int64_t s) { return n >= 0 && n <= kFpsMaxRows && s >= 0 && s <= kFpsMaxSegments; }

}  // namespace

}  // namespace lgs

using namespace lgs;

extern "C" {

int64_t lgs_fps_workspace_bytes(int64_t n, int64_t s) {
  if (!fps_shape_ok(n, s)) return 0;
  return fps_layout(n, s).total;
}

int lgs_fps_segments(const float *points, int64_t n, const int64_t *through, const int64_t *seg_offsets, int64_t s,
                     const int32_t *counts, int fixed_count, double ratio, int min_points, int skip_origin,
                     const int64_t *out_offsets, int32_t *idx_out, int32_t *rank_out, void *workspace, void *stream) {
  LGS_REQUIRE(fps_shape_ok(n, s), "lgs_fps_segments: 0 <= n < 2^31 - 1 rows and 0 <= s <= 2^20 segments");
  LGS_REQUIRE(seg_offsets && workspace && (n == 0 || points), "lgs_fps_segments: bad argument");
  LGS_REQUIRE(idx_out || rank_out, "lgs_fps_segments: neither idx_out nor rank_out");
  if (!counts && fixed_count < 0)
    LGS_REQUIRE(ratio >= 0.0 && ratio <= 1.0 && min_points >= 0 && min_points <= (1 << 24),
                "lgs_fps_segments: the count rule needs 0 <= ratio <= 1 and 0 <= min_points <= 2^24");
  LGS_REQUIRE(!idx_out || out_offsets || (!counts && fixed_count >= 0),
              "lgs_fps_segments: idx_out needs out_offsets, or a fixed count (segment q writes at q * fixed_count)");
  hipStream_t st = (hipStream_t)stream;
  const FpsWs w = fps_layout(n, s);
  FpsSeg *segs = Layout::at<FpsSeg>(workspace, w.segs);
  float4 *state = Layout::at<float4>(workspace, w.state);
  if (rank_out && n > 0) LGS_KLAUNCH(k_fps_fill, (unsigned)((n + 255) / 256), 256, 0, st, rank_out, n);
  if (s > 0 && n > 0) {
    LGS_KLAUNCH(k_fps_table, 1, kFpsTableBlock, 0, st, seg_offsets, n, s, counts, fixed_count, ratio, min_points, out_offsets, segs);
    LGS_KLAUNCH(k_fps_wave, (unsigned)((s + 3) / 4), 256, 0, st, points, n, through, segs, s, skip_origin, idx_out, rank_out);
    LGS_KLAUNCH(k_fps_group<4>, (unsigned)s, 256, 0, st, points, n, through, segs, kFpsWaveMax, kFpsGroup4Max, skip_origin, idx_out,
                rank_out);
    LGS_KLAUNCH(k_fps_group<16>, (unsigned)s, 1024, 0, st, points, n, through, segs, kFpsGroup4Max, kFpsGroup16Max, skip_origin, idx_out,
                rank_out);
    if (n > kFpsGroup16Max)
      LGS_KLAUNCH(k_fps_stream, (unsigned)s, kFpsStreamWaves * 64, 0, st, points, n, through, segs, kFpsGroup16Max, skip_origin, state,
                  idx_out, rank_out);
  }
  LGS_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
